/*
 * ucfp_hip.h -- C ABI of the MI355X (gfx950) fingerprint + brute-force ANN core.
 *
 * This is the drop-in boundary for the UCFP hot path.  The reference has no FFI
 * today (it calls three crates.io SDKs in-process); each entry point below names
 * the Rust seam it replaces, as /root/reference/<file>:<line>.  A Rust host binds
 * these with `extern "C"`; this repo's Python host binds them
 * with ctypes (ucfp_amd/_lib.py).
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types.
 *   - `*_dev` entry points take DEVICE pointers and a hipStream_t (as void*); they
 *     enqueue work and return without synchronising.  The non-`_dev` variants take
 *     HOST pointers, stage through the context's device workspace and block until
 *     the result is in the caller's buffer (they mirror the per-request reference
 *     call: borrowed input, owned output copy -- src/modality/image.rs:82).
 *   - return value: 0 (UCFP_OK) or a negative ucfp_status.  Per-item failures of a
 *     batch are reported in `status[i]` and do not fail the call.
 *   - a context is thread-safe for concurrent calls on distinct streams; the error
 *     string is per-thread.
 */
#ifndef UCFP_HIP_H
#define UCFP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UCFP_ABI_VERSION 2

/* ---- status codes: map 1:1 onto the reference's Error enum (src/error.rs:9-61,
 *      HTTP mapping src/server/error.rs:22-41) ------------------------------------ */
typedef enum ucfp_status {
    UCFP_OK = 0,
    UCFP_E_MODALITY = -1,    /* Error::Modality  -> 400: bad input for the algorithm  */
    UCFP_E_UNSUPPORTED = -2, /* Error::Unsupported -> 501: algorithm/option not built */
    UCFP_E_INDEX = -3,       /* Error::Index -> 500: device / runtime failure         */
    UCFP_E_INVALID = -4,     /* null pointer, bad enum, size overflow (caller bug)    */
    UCFP_E_NOT_FOUND = -5    /* Error::RecordNotFound -> 404                          */
} ucfp_status;

typedef struct ucfp_ctx ucfp_ctx;

/* Create a context bound to HIP device `device_id` (one process per GPU: the caller
 * passes LOCAL_RANK).  Fails with UCFP_E_INDEX when no gfx950 device is usable --
 * there is deliberately no CPU fallback. */
int ucfp_ctx_create(int device_id, ucfp_ctx** out);
void ucfp_ctx_destroy(ucfp_ctx* ctx);
/* Thread-local UTF-8 message of the last failing call (the `String` payload of
 * Error::Modality / Error::Index). Never NULL. */
const char* ucfp_last_error(void);
int ucfp_abi_version(void);

/* =============================== IMAGE ========================================
 * Replaces the arithmetic behind
 *   image::fingerprint_with            src/modality/image.rs:62-88   (multi, 536 B)
 *   image::fingerprint_{p,d,a}hash     src/modality/image.rs:112-194 (single, 168 B)
 * i.e. imgfprint::ImageFingerprinter::fingerprint_with_preprocess and
 * FingerprinterContext::fingerprint_with_algorithm_and_preprocess, AFTER decode.
 * Input is a batch of decoded frames of one geometry.
 */
typedef enum ucfp_pixfmt {
    UCFP_PIX_GRAY8 = 0, /* 1 byte / pixel, luma                                  */
    UCFP_PIX_RGB8 = 1,  /* 3 bytes / pixel, R,G,B                                */
    UCFP_PIX_RGBA8 = 2  /* 4 bytes / pixel, alpha ignored                        */
} ucfp_pixfmt;

typedef enum ucfp_image_algo {
    UCFP_IMG_AHASH = 1, /* ?algorithm=ahash  tag imgfprint-ahash-v1              */
    UCFP_IMG_PHASH = 2, /* ?algorithm=phash  tag imgfprint-phash-v1              */
    UCFP_IMG_DHASH = 4, /* ?algorithm=dhash  tag imgfprint-dhash-v1              */
    UCFP_IMG_MULTI = 7  /* ?algorithm=multi  tag imgfprint-multihash-v1          */
} ucfp_image_algo;

#define UCFP_IMAGE_FP_BYTES 168    /* imgfprint::ImageFingerprint, repr(C)        */
#define UCFP_IMAGE_MULTI_BYTES 536 /* imgfprint::MultiHashFingerprint, repr(C)    */
#define UCFP_IMAGE_NORM 256        /* side of the normalised luma plane           */

/* imgfprint::PreprocessConfig guards (defaults: src/server/algorithms_manifest.rs:446-469;
 * query mapping src/server/handlers.rs:307-319).  max_input_bytes concerns the ENCODED
 * payload and is enforced by the host before decode. */
typedef struct ucfp_image_preprocess {
    uint32_t max_dimension; /* default 8192 */
    uint32_t min_dimension; /* default 32   */
} ucfp_image_preprocess;

/* Bytes of one output record for `algo` (168 for a single algorithm, 536 for MULTI;
 * 0 for an invalid mask). */
size_t ucfp_image_record_bytes(uint32_t algo);

/* 64-bit global hashes of n stored image records -> Hamming codes for ucfp_index_append_dev (byte
 * offset 32 of a 168-byte record, 32 + {32, 200, 368} of the 536-byte bundle).  `algo` names the record type,
 * `which` (AHASH / PHASH / DHASH) the member of a MULTI bundle; ignored otherwise. */
int ucfp_image_record_codes_dev(ucfp_ctx* ctx, const uint8_t* d_records, size_t n, uint32_t algo, uint32_t which,
                                uint64_t* d_codes, void* stream);

/* Device-resident batch.
 *   frames      n frames; frame i starts at frames + i*frame_stride, row y at
 *               + y*row_stride; pixels packed per `pixfmt`. 16-byte aligned base and
 *               strides take the vectorised path.
 *   exact       n x 32 bytes: BLAKE3 of each ORIGINAL encoded image, computed by the
 *               host that still has those bytes (the reference hashes the upload,
 *               not the pixels); NULL writes zeros.
 *   out         n x ucfp_image_record_bytes(algo), layout exactly the reference's
 *               bytemuck::bytes_of(&fp) (image.rs:82,188).
 *   status      n x int32 (may be NULL): 0 or UCFP_E_MODALITY per frame.
 * Geometry violations of `pre` fail every frame of the batch (all share w,h). */
int ucfp_image_hash_batch_dev(ucfp_ctx* ctx, uint32_t algo, const uint8_t* frames, size_t n,
                              uint32_t width, uint32_t height, size_t row_stride,
                              size_t frame_stride, int pixfmt,
                              const ucfp_image_preprocess* pre, const uint8_t* exact,
                              uint8_t* out, int32_t* status, void* stream);

/* Host-pointer variant (per-request path: n is usually 1). Same arguments, host memory. */
int ucfp_image_hash_batch(ucfp_ctx* ctx, uint32_t algo, const uint8_t* frames, size_t n,
                          uint32_t width, uint32_t height, size_t row_stride,
                          size_t frame_stride, int pixfmt, const ucfp_image_preprocess* pre,
                          const uint8_t* exact, uint8_t* out, int32_t* status);

/* RAGGED batch of decoded frames: every frame has its own geometry -- the reference's image route takes any upload
 * (src/server/handlers.rs:232-302 -> src/modality/image.rs:54-88: "PNG / JPEG / WebP / GIF / BMP", any size), so what a
 * server hands over after decode is a mix of sizes.  Frame i is described by items[i] (a HOST array; the library plans
 * the launch from it): its first pixel sits `offset` bytes into `frames`, rows `row_stride` bytes apart, `pixfmt` pixels.
 * One launch per form of row (up to / beyond 512 pixels) hashes the whole batch: a workgroup takes a frame from source
 * bytes to record with the 256 x 256 normalised plane kept in registers and LDS, never in memory.  Outputs as
 * ucfp_image_hash_batch_dev, indexed like `items`; a frame outside the guards of `pre` (or of zero size) gets
 * status[i] = UCFP_E_MODALITY and a zero record, the others are unaffected.  frames_bytes: the readable bytes behind
 * `frames` (the unaligned loader reads whole dwords, never outside them). */
typedef struct ucfp_image_item {
    uint64_t offset;     /* first pixel of the frame, bytes from `frames`                 */
    uint32_t width, height;
    uint32_t row_stride; /* bytes; >= width x bytes per pixel                              */
    int32_t pixfmt;      /* ucfp_pixfmt                                                    */
} ucfp_image_item;
int ucfp_image_hash_ragged_dev(ucfp_ctx* ctx, uint32_t algo, const uint8_t* d_frames, size_t frames_bytes,
                               const ucfp_image_item* items, size_t n, const ucfp_image_preprocess* pre, const uint8_t* d_exact,
                               uint8_t* d_out, int32_t* d_status, void* stream);
/* Host-pointer variant: frames / exact / out / status in host memory; blocks until the records are in `out`. */
int ucfp_image_hash_ragged(ucfp_ctx* ctx, uint32_t algo, const uint8_t* frames, size_t frames_bytes, const ucfp_image_item* items,
                           size_t n, const ucfp_image_preprocess* pre, const uint8_t* exact, uint8_t* out, int32_t* status);

/* ---- encoded uploads of any size and format in one batch (SURVEY 8f N1 + N4) ----
 * What the reference's route receives (src/server/handlers.rs:232-302) is an encoded file of unknown kind and size, decoded
 * inside the SDK call (src/modality/image.rs:68-70).  ucfp_image_probe tells from the first bytes what it is and what frame
 * it decodes to; the batch entries below take files of ANY mix of kinds and sizes: PNG and baseline JPEG are decoded on
 * the device (scope: the PNG / JPEG front-end sections below), everything else -- WebP, GIF, BMP, the PNG and JPEG kinds the
 * device hands back -- gets status UCFP_IMAGE_NEEDS_HOST and goes to the host's decoder. */
#define UCFP_IMAGE_NEEDS_HOST 1
typedef enum ucfp_upload_format {
    UCFP_UPLOAD_OTHER = 0, /* not PNG / JPEG: the host's decoder decides                    */
    UCFP_UPLOAD_PNG = 1,
    UCFP_UPLOAD_JPEG = 2
} ucfp_upload_format;
typedef struct ucfp_upload_info {
    int32_t format;        /* ucfp_upload_format                                             */
    int32_t status;        /* UCFP_OK: the device decodes it; UCFP_IMAGE_NEEDS_HOST; UCFP_E_MODALITY */
    uint32_t width, height;
    int32_t pixfmt;        /* the frame the file decodes to (a JPEG: its luma plane, GRAY8)   */
    uint32_t reserved;
} ucfp_upload_info;
/* Host-side, on the upload's own bytes (a request thread calls it before submitting): fills *info, returns info->status. */
int ucfp_image_probe(const uint8_t* bytes, size_t len, ucfp_upload_info* info);
/* The same for uploads that are already in device memory (one blob + n + 1 byte offsets, like the text calls): d_info
 * receives n entries.  No synchronisation. */
int ucfp_image_probe_batch_dev(ucfp_ctx* ctx, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n, ucfp_upload_info* d_info,
                               void* stream);
/* Encoded uploads of ANY mix of kinds and sizes -> records.  info: n probe results in HOST memory (the library plans the
 * launches and sizes its workspace from them; every file's own header is checked against its entry on the device, a
 * mismatch is UCFP_IMAGE_NEEDS_HOST) -- or NULL: the files are probed on the device first, which costs one host
 * synchronisation inside the call.  PNG files are inflated and unfiltered, JPEG files Huffman-decoded and inverse-
 * transformed (luma plane) into frames of their own sizes in the context's workspace, BLAKE3 of every file is computed
 * when d_exact is NULL, and ONE ragged hash (ucfp_image_hash_ragged_dev's kernels) makes the records.  status[i]: 0,
 * UCFP_IMAGE_NEEDS_HOST (not PNG / JPEG, or a kind of them the device hands back, or a decode irregularity: the host's
 * decoder decides), UCFP_E_MODALITY (damaged file; geometry outside `pre`); records of files with a non-zero status are
 * zero.  blob_bytes = d_offsets[n]. */
int ucfp_image_upload_hash_batch_dev(ucfp_ctx* ctx, uint32_t algo, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n,
                                     size_t blob_bytes, const ucfp_upload_info* info, const ucfp_image_preprocess* pre,
                                     const uint8_t* d_exact, uint8_t* d_out, int32_t* d_status, void* stream);
/* Decode only: frames into the caller's buffer (16-byte aligned, ucfp_image_upload_frames_bytes(info, n) bytes), laid out
 * by the library; items[i] (HOST, n entries) receives where frame i is and its geometry (width 0: not decoded) -- ready for
 * ucfp_image_hash_ragged_dev. */
size_t ucfp_image_upload_frames_bytes(const ucfp_upload_info* info, size_t n);
int ucfp_image_upload_decode_batch_dev(ucfp_ctx* ctx, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n, size_t blob_bytes,
                                       const ucfp_upload_info* info, uint8_t* d_frames, size_t frames_bytes, ucfp_image_item* items,
                                       int32_t* d_status, void* stream);

/* Host micro-batcher for uploads of ANY kind and size (SURVEY 8f N1 + N4): the per-request shape of handlers::ingest_image
 * (src/server/handlers.rs:232-302: one upload per request thread, up to 512 in flight, src/bin/ucfp.rs:267) with NO geometry
 * or format announced at creation.  submit() is BLOCKING and thread-safe: the calling thread probes its own bytes
 * (ucfp_image_probe); what the device does not decode returns at once with *status = UCFP_IMAGE_NEEDS_HOST / UCFP_E_MODALITY
 * and a zero record; everything else -- PNG and JPEG files of whatever sizes -- is coalesced with the other threads'
 * uploads into ONE H2D copy + ucfp_image_upload_hash_batch_dev (decode, BLAKE3 of the file, ragged hash) + one D2H copy
 * of the records, at most max_batch uploads / max_bytes encoded bytes per flush, flushed no later than max_delay_us after
 * the first pending upload.  Inside, PNG and JPEG uploads coalesce in two lanes (each with max_batch / max_bytes of its own;
 * the JPEG lane on a context the batcher creates for itself), so that a JPEG request -- a few milliseconds of decode -- does
 * not wait for the largest PNG of a shared flush -- tens of milliseconds, its LZ77 pass being one wave's serial work. */
typedef struct ucfp_upload_batcher ucfp_upload_batcher;
int ucfp_upload_batcher_create(ucfp_ctx* ctx, uint32_t algo, const ucfp_image_preprocess* pre, size_t max_batch, size_t max_bytes,
                               uint32_t max_delay_us, ucfp_upload_batcher** out);
void ucfp_upload_batcher_destroy(ucfp_upload_batcher* b);
int ucfp_upload_batcher_submit(ucfp_upload_batcher* b, const uint8_t* bytes, size_t len, uint8_t* out, int32_t* status);
int ucfp_upload_batcher_stats(ucfp_upload_batcher* b, uint64_t* batches, uint64_t* items);

/* ---- PNG front end ----
 * The reference decodes the upload inside the SDK call (src/modality/image.rs:68-70, :176-179: imgfprint ->
 * image::load_from_memory); BASELINE config 1 (1 k 256x256 PNGs) is decode-bound on the CPU.  These entry points take
 * the ENCODED files: one blob + n + 1 byte offsets (like the text calls), all announced with ONE geometry and pixel
 * format -- the host reads those 24 bytes of each upload with ucfp_png_probe and groups by them.  One wave per file:
 * chunk walk, inflate (RFC 1950/1951, speculative parallel Huffman decoding), PNG filter reconstruction.
 * Decoded on the device: 8-bit, non-interlaced -- greyscale and grey + alpha (-> GRAY8, the alpha byte is dropped: luma
 * takes no alpha), RGB and indexed colour (-> RGB8 through the file's PLTE), RGBA (-> RGBA8), each with or without a tRNS
 * chunk (simple transparency only adds an alpha channel: no colour sample changes); files of both layouts of a format may
 * share a batch.  ucfp_png_probe reports the format a file DECODES to.  status[i]:
 *   0                      decoded (and hashed)
 *   UCFP_IMAGE_NEEDS_HOST  a valid PNG of another kind (16-bit, 1/2/4-bit, interlaced) or of another geometry /
 *                          format than announced, or a file whose only fault is a CHECKSUM (the Adler-32 of a stream that
 *                          inflated to the right length, the CRC of an ancillary chunk): decoders differ on those, so
 *                          the host's decoder decides -- decode it there, submit the pixels
 *   UCFP_E_MODALITY        not a PNG / damaged stream / bad CRC on a critical chunk (the reference answers 400)
 * png_bytes = d_offsets[n] (the host knows it; sizes the context's workspace: about png_bytes + n x (2 x frame bytes)). */
/* Host-side: geometry and pixel format of a PNG from its IHDR.  UCFP_OK, UCFP_IMAGE_NEEDS_HOST or UCFP_E_MODALITY. */
int ucfp_png_probe(const uint8_t* png, size_t len, uint32_t* width, uint32_t* height, int* pixfmt);
/* Encoded files -> frames (frame i at d_frames + i*frame_stride, rows row_stride apart). */
int ucfp_image_png_decode_batch_dev(ucfp_ctx* ctx, const uint8_t* d_png, const uint64_t* d_offsets, size_t n,
                                    size_t png_bytes, uint32_t width, uint32_t height, int pixfmt, uint8_t* d_frames,
                                    size_t row_stride, size_t frame_stride, int32_t* d_status, void* stream);
/* Encoded files -> records: decode into the context's workspace, then ucfp_image_hash_batch_dev's kernels.
 * d_exact: n x 32 bytes, BLAKE3 of each file as computed by the host -- or NULL: the files are on the device, so their
 * BLAKE3 is computed there (ucfp_blake3_batch_dev's kernel).  Records of files that did not decode are zero. */
int ucfp_image_png_hash_batch_dev(ucfp_ctx* ctx, uint32_t algo, const uint8_t* d_png, const uint64_t* d_offsets, size_t n,
                                  size_t png_bytes, uint32_t width, uint32_t height, int pixfmt,
                                  const ucfp_image_preprocess* pre, const uint8_t* d_exact, uint8_t* d_out,
                                  int32_t* d_status, void* stream);

/* Host micro-batcher for ENCODED uploads (SURVEY 8f N1 + N4): the per-request shape of handlers::ingest_image
 * (src/server/handlers.rs:232-302) with the decode moved to the device.  One batcher per announced geometry and pixel
 * format (ucfp_png_probe tells them from the first 29 bytes); concurrent submit() calls become ONE H2D copy of the
 * encoded bytes + ucfp_image_png_hash_batch_dev (PNG decode, BLAKE3 of the file, hashing) + one D2H copy of the
 * records.  *status as there: UCFP_IMAGE_NEEDS_HOST -> decode that upload on the host and use ucfp_image_batcher_submit. */
typedef struct ucfp_png_batcher ucfp_png_batcher;
int ucfp_png_batcher_create(ucfp_ctx* ctx, uint32_t algo, uint32_t width, uint32_t height, int pixfmt,
                            const ucfp_image_preprocess* pre, size_t max_batch, size_t max_bytes, uint32_t max_delay_us,
                            ucfp_png_batcher** out);
void ucfp_png_batcher_destroy(ucfp_png_batcher* b);
int ucfp_png_batcher_submit(ucfp_png_batcher* b, const uint8_t* png, size_t len, uint8_t* out, int32_t* status);
int ucfp_png_batcher_stats(ucfp_png_batcher* b, uint64_t* batches, uint64_t* items);

/* BLAKE3 (32-byte digests) of n byte strings that are already on the device: one blob + n + 1 byte offsets, like the
 * text calls; blob_bytes = d_offsets[n]; the blob must be readable up to the next multiple of 4 bytes.  This is the
 * records' `exact` field (image.rs:82: BLAKE3 of the upload) for uploads that were copied to the device encoded.
 * Host-side single input: ucfp_blake3. */
int ucfp_blake3_batch_dev(ucfp_ctx* ctx, const uint8_t* d_blob, const uint64_t* d_offsets, size_t n, size_t blob_bytes,
                          uint8_t* d_out, void* stream);

/* Host micro-batcher: the caller side of handlers::ingest_image
 * (src/server/handlers.rs:232-302) hashes one image per request thread, up to 512 in flight
 * (src/bin/ucfp.rs:267).  submit() is BLOCKING and thread-safe: concurrent calls are coalesced
 * into one pinned-memory copy + one launch of at most max_batch frames, flushed no later than
 * max_delay_us after the first pending frame arrived.  One geometry per batcher. */
typedef struct ucfp_image_batcher ucfp_image_batcher;
int ucfp_image_batcher_create(ucfp_ctx* ctx, uint32_t algo, uint32_t width, uint32_t height, int pixfmt,
                              const ucfp_image_preprocess* pre, size_t max_batch, uint32_t max_delay_us,
                              ucfp_image_batcher** out);
void ucfp_image_batcher_destroy(ucfp_image_batcher* b);
int ucfp_image_batcher_submit(ucfp_image_batcher* b, const uint8_t* frame, size_t row_stride,
                              const uint8_t* exact, uint8_t* out, int32_t* status);
int ucfp_image_batcher_stats(ucfp_image_batcher* b, uint64_t* batches, uint64_t* items);

/* Synthetic workload of SURVEY 8(d) config 2, generated on device: frame i, pixel (x,y) =
 * ((x + y + 17*i) & 255) ^ (splitmix64((i*h + y)*w + x) >> 60): a ramp with 4 bits of seeded
 * noise. Deterministic; the oracle has the same generator. Bench/test support only. */
int ucfp_image_synth_dev(ucfp_ctx* ctx, uint8_t* frames, size_t n, uint32_t width,
                         uint32_t height, size_t first_index, void* stream);

/* =============================== AUDIO ========================================
 * Replaces the arithmetic behind
 *   audio::fingerprint_wang_with      src/modality/audio.rs:64-98    ([WangHash], 8 B each)
 *   audio::fingerprint_haitsma_with   src/modality/audio.rs:181-224  (u32 per frame)
 * i.e. audiofp::classical::{Wang, Haitsma}::extract and audiofp::dsp::resample::linear.
 * Input: mono f32 PCM.  Wang requires 8 kHz (audio.rs:422-430) -- other rates are rejected with
 * UCFP_E_MODALITY; resample upstream (ucfp_audio_resample_linear*).  Haitsma resamples to 5 kHz
 * itself, like the reference (audio.rs:194-200).
 */
typedef struct ucfp_wang_config { /* audiofp WangConfig; defaults algorithms_manifest.rs:553-592 */
    uint32_t fan_out;          /* 10  */
    uint32_t target_zone_t;    /* 63 frames */
    uint32_t target_zone_f;    /* 64 bins   */
    uint32_t peaks_per_sec;    /* 30  */
    float min_anchor_mag_db;   /* -50 (dB re full-scale sine) */
} ucfp_wang_config;

typedef struct ucfp_haitsma_config { /* audiofp HaitsmaConfig; defaults manifest :655-672 */
    float fmin; /* 300  */
    float fmax; /* 2000 */
} ucfp_haitsma_config;

#define UCFP_WANG_HASH_BYTES 8 /* u32 LE f_a(9)|f_b(9)|dt(14), u32 LE t_anchor (LandmarkScatter.svelte:4) */

/* Upper bound on the hashes n samples can produce (for sizing `out`). */
size_t ucfp_audio_wang_max_hashes(size_t n_samples, const ucfp_wang_config* cfg);
/* Host buffers; *n_hashes receives the number produced (if it exceeds cap_hashes the output is
 * truncated and UCFP_E_INVALID is returned). cfg NULL = defaults. */
int ucfp_audio_wang(ucfp_ctx* ctx, const float* pcm, size_t n, uint32_t sample_rate, const ucfp_wang_config* cfg,
                    uint8_t* out, size_t cap_hashes, size_t* n_hashes);
/* Device buffers; d_n_hashes is a device u64 (total produced, may exceed cap). No sync. */
int ucfp_audio_wang_dev(ucfp_ctx* ctx, const float* d_pcm, size_t n, uint32_t sample_rate,
                        const ucfp_wang_config* cfg, uint8_t* d_out, size_t cap_hashes, uint64_t* d_n_hashes,
                        void* stream);

/* RAGGED BATCH of clips (SURVEY 8f N1 for audio: the reference ingests one short clip per request,
 * src/server/handlers.rs:704-918; its bench clip is 4 s, benches/end_to_end.rs:55-75): clip i is
 * d_pcm[d_offsets[i] .. d_offsets[i+1]) (n_clips + 1 device u64 offsets, d_offsets[n_clips] <= n_total), all at
 * `sample_rate`.  8000 Hz clips are taken as they are; any other rate is resampled to 8 kHz by
 * audiofp::dsp::resample::linear (A1) INSIDE the kernel that cuts the STFT frames -- HBM sees every source sample
 * once (BASELINE config 3: 44.1 kHz).  One launch sequence covers the whole batch.  Hashes of clip i land in
 * d_out[d_out_offsets[i] .. d_out_offsets[i+1]) (8 bytes each, t_anchor relative to the clip); d_out_offsets has
 * n_clips + 1 device u64 entries; if d_out_offsets[n_clips] > cap_hashes the output was truncated at cap_hashes.
 * Workspace: about 4 KiB per second of audio in the batch, held by the context.  No synchronisation. */
size_t ucfp_audio_wang_batch_max_hashes(size_t n_total, size_t n_clips, uint32_t sample_rate, const ucfp_wang_config* cfg);
int ucfp_audio_wang_batch_dev(ucfp_ctx* ctx, const float* d_pcm, const uint64_t* d_offsets, size_t n_total, size_t n_clips,
                              uint32_t sample_rate, const ucfp_wang_config* cfg, uint8_t* d_out, size_t cap_hashes,
                              uint64_t* d_out_offsets, void* stream);

/* PANAKO triplets: audio::fingerprint_panako / fingerprint_panako_with (src/modality/audio.rs:106-156,
 * the seam is the extract call at audio.rs:136-139) behind ?algorithm=panako (src/server/handlers.rs:778-836).  The
 * front end is Wang's (8 kHz, 1024 / 128 STFT, 62.5 frames/s, peaks_per_sec strongest peaks per second); an anchor above
 * the magnitude floor joins PAIRS of peaks of its target zone into triplets (a, b, c), at most fan_out per anchor.
 * A record is 16 bytes, little-endian: u32 hash = f_a(9) | f_b(9) | f_c(9) | r(5) with r = min(31, 32 (t_b - t_a) /
 * (t_c - t_a)), then u32 t_anchor, u32 t_b, u32 t_c in frames (LandmarkScatter.svelte:5, :31-35).  Output buffers
 * must be 16-byte aligned (UCFP_E_INVALID otherwise).  The entries mirror the Wang ones: same limits, same errors. */
typedef struct ucfp_panako_config { /* audiofp PanakoConfig; defaults and ranges algorithms_manifest.rs:601-650 */
    uint32_t fan_out;          /* 5   (1 .. 64)   triplets per anchor */
    uint32_t target_zone_t;    /* 96  (1 .. 512)  frames */
    uint32_t target_zone_f;    /* 96  (1 .. 1024) bins */
    uint32_t peaks_per_sec;    /* 30  (1 .. 256) */
    float min_anchor_mag_db;   /* -50 (-120 .. 0, dB re full-scale sine) */
} ucfp_panako_config;

#define UCFP_PANAKO_HASH_BYTES 16 /* u32 LE hash, t_anchor, t_b, t_c (LandmarkScatter.svelte:5, AlgorithmView.svelte:134) */

/* Upper bound on the records n samples at 8 kHz can produce: seconds * peaks_per_sec * fan_out. */
size_t ucfp_audio_panako_max_hashes(size_t n_samples, const ucfp_panako_config* cfg);
/* Host buffers, 8 kHz only (UCFP_E_MODALITY otherwise, src/server/tests.rs:391); *n_hashes receives the number produced
 * (if it exceeds cap_hashes the output is truncated and UCFP_E_INVALID is returned). cfg NULL = defaults. */
int ucfp_audio_panako(ucfp_ctx* ctx, const float* pcm, size_t n, uint32_t sample_rate, const ucfp_panako_config* cfg,
                      uint8_t* out, size_t cap_hashes, size_t* n_hashes);
/* Device buffers; d_n_hashes is a device u64 (total produced, may exceed cap). No sync. */
int ucfp_audio_panako_dev(ucfp_ctx* ctx, const float* d_pcm, size_t n, uint32_t sample_rate,
                          const ucfp_panako_config* cfg, uint8_t* d_out, size_t cap_hashes, uint64_t* d_n_hashes,
                          void* stream);
/* Ragged batch, as ucfp_audio_wang_batch_dev: clip i = d_pcm[d_offsets[i] .. d_offsets[i+1]) at `sample_rate`
 * (1 000 .. 384 000 Hz; resampled to 8 kHz inside the kernel unless it is 8000).  Records of clip i land in
 * d_out[d_out_offsets[i] .. d_out_offsets[i+1]) (16 B each, times relative to the clip); a triplet never crosses a clip
 * boundary.  d_out_offsets[n_clips] > cap_hashes: truncated at cap_hashes.  No synchronisation. */
size_t ucfp_audio_panako_batch_max_hashes(size_t n_total, size_t n_clips, uint32_t sample_rate,
                                          const ucfp_panako_config* cfg);
int ucfp_audio_panako_batch_dev(ucfp_ctx* ctx, const float* d_pcm, const uint64_t* d_offsets, size_t n_total,
                                size_t n_clips, uint32_t sample_rate, const ucfp_panako_config* cfg, uint8_t* d_out,
                                size_t cap_hashes, uint64_t* d_out_offsets, void* stream);

/* Host micro-batcher for clips (audio): one clip per request thread (handlers.rs:704-918); concurrent
 * submit() calls become ONE ucfp_audio_wang_batch_dev call over at most max_batch clips / max_samples samples, flushed
 * no later than max_delay_us after the first pending clip.  All clips at `sample_rate` (resampled to 8 kHz in the
 * kernel).  *n_hashes = hashes of this clip (t_anchor relative to the clip); more than cap_hashes -> UCFP_E_INVALID
 * with the first cap_hashes written (as ucfp_audio_wang). */
typedef struct ucfp_audio_batcher ucfp_audio_batcher;
int ucfp_audio_batcher_create(ucfp_ctx* ctx, uint32_t sample_rate, const ucfp_wang_config* cfg, size_t max_batch,
                              size_t max_samples, uint32_t max_delay_us, ucfp_audio_batcher** out);
void ucfp_audio_batcher_destroy(ucfp_audio_batcher* b);
int ucfp_audio_batcher_submit(ucfp_audio_batcher* b, const float* pcm, size_t n, uint8_t* out, size_t cap_hashes,
                              size_t* n_hashes);
int ucfp_audio_batcher_stats(ucfp_audio_batcher* b, uint64_t* batches, uint64_t* items);

/* STREAMING Wang: audio::StreamingWangSession::new / push / finalize (src/modality/audio.rs:413-480)
 * behind POST /v1/ingest/audio/{tid}/{rid}/stream (src/server/handlers.rs:957-1010), with the state on the device and
 * many streams advanced by one push.  A set holds max_streams slots; a slot is one stream at 8 kHz.  The Wang spec is
 * local in time, so after a push that brings a stream to n samples the hashes emitted so far are exactly the offline
 * hashes (ucfp_audio_wang on the same samples) with t_anchor < F(n) (ucfp_wang_stream_frontier), in offline order; a
 * final push emits the rest.  The concatenation over all pushes equals ucfp_audio_wang of the whole stream byte for
 * byte, however the stream is cut into chunks.  t_anchor counts frames since the stream was opened (u32, ~795 days;
 * the 2^23-frame limit of one offline clip does not apply).  With the default config the emission lag is at most
 * 7 + 62 + 63 = 132 frames (2.1 s).
 *   - The set serialises its own calls: it is safe to call from several threads.  Consecutive pushes are ordered by
 *     the set itself (an event), whatever `stream` the caller passes.
 *   - Device bytes per stream: ucfp_wang_streams_state_bytes(cfg) (about 16.5 KiB with the defaults: 2816 carried
 *     samples, the open second's <= 320 candidates, the retained peaks), fixed at creation, whatever the stream's
 *     length.  The push path allocates nothing beyond growing the context's workspace to the largest push seen.
 *   - Errors are status codes: UCFP_E_INVALID for a slot out of range or not open, a slot twice in one push, a chunk
 *     above 2^29 samples, a stream that would pass 2^32 frames, cap_hashes below the bound; UCFP_E_MODALITY for a rate
 *     other than 8000 or a config outside the /v1/algorithms ranges.  A failed call changes no state.
 *   - LIVE WINDOWS (the reference has no audio matcher): a set created by ucfp_wang_streams_create_ex
 *     with window_frames = W (0 .. UCFP_WANG_STREAM_MAX_WINDOW_FRAMES; 0 = no windows, the set of
 *     ucfp_wang_streams_create exactly) also keeps each stream's latest hashes for ucfp_landmark_index_query*.  The
 *     window of an open stream at n samples is its emitted hashes with t_anchor >= w0 = max(0, F(n) - W), in emission
 *     order, with w0 subtracted from t_anchor; at most ucfp_wang_streams_window_cap(cfg, W) = (ceil(2 W / 125) + 1) *
 *     peaks_per_sec * fan_out hashes.  Nothing pushed or emitted yet, a final push or close: empty, origin 0.  A hit's
 *     `offset` then says where stream frame w0 lies in the matched record.  W above the maximum, a misaligned
 *     landmark buffer, a windows call on a set without windows: UCFP_E_INVALID. */
typedef struct ucfp_wang_streams ucfp_wang_streams;
#define UCFP_WANG_STREAM_MAX_WINDOW_FRAMES 8192u /* 131 s */
/* sample_rate must be 8000 (audio.rs:425-431 -> UCFP_E_MODALITY); cfg as ucfp_audio_wang, NULL = defaults.  The rate and
 * the config are checked before anything else.  Fails with UCFP_E_INDEX without a gfx950 device (no CPU fallback). */
int ucfp_wang_streams_create(ucfp_ctx* ctx, uint32_t sample_rate, const ucfp_wang_config* cfg, uint32_t max_streams,
                             ucfp_wang_streams** out);
/* StreamingWangSession::new (audio.rs:413-431) for a set that also keeps live windows of window_frames frames (A20; the
 * reference has no audio matcher).  window_frames = 0 is ucfp_wang_streams_create; above the maximum: UCFP_E_INVALID,
 * after the rate and the config (UCFP_E_MODALITY). */
int ucfp_wang_streams_create_ex(ucfp_ctx* ctx, uint32_t sample_rate, const ucfp_wang_config* cfg, uint32_t max_streams,
                                uint32_t window_frames, ucfp_wang_streams** out);
/* A set that takes its feed at ANY rate from 1 000 to 384 000 Hz and resamples it on the device (the
 * reference resamples upstream of the session).  A stream that has received n input samples holds S(n) final 8 kHz
 * samples (ucfp_wang_stream_samples); everything above then holds with S(n) in n's place: the hashes emitted so far
 * are the offline hashes at that rate (ucfp_audio_wang_batch_dev over the one clip) with t_anchor <
 * ucfp_wang_stream_frontier(S(n)), and the concatenation over all pushes equals that offline record byte for byte,
 * however the feed is cut -- empty chunks, one-sample chunks and chunks that release no 8 kHz sample included.
 * n_samples of open / push / push_dev / max_hashes count INPUT samples; t_anchor, the window origins and W stay in
 * 8 kHz frames.  On top of the state above a slot carries the <= ceil(sample_rate / 8000) + 1 input samples the next
 * 8 kHz sample needs.  A rate outside the range: UCFP_E_MODALITY ("sample rate"), judged with the config before
 * anything else.  At 8000 this is ucfp_wang_streams_create_ex exactly.  A chunk is at most 2^29 input samples and may
 * release at most 2^29 samples at 8 kHz: UCFP_E_INVALID otherwise, before any state changes. */
int ucfp_wang_streams_create_sr(ucfp_ctx* ctx, uint32_t sample_rate, const ucfp_wang_config* cfg, uint32_t max_streams,
                                uint32_t window_frames, ucfp_wang_streams** out);
void ucfp_wang_streams_destroy(ucfp_wang_streams* s);
int ucfp_wang_streams_open(ucfp_wang_streams* s, uint32_t* slot);      /* fresh stream, t = 0 (audio.rs:413-431) */
int ucfp_wang_streams_close(ucfp_wang_streams* s, uint32_t slot);      /* discard, emit nothing */
/* Host-only, no GPU: F(n) of A9 -- frames(n) = n < 1024 ? 0 : (n - 1024) / 128 + 1, J = max(0, frames - 7),
 * C = the first frame of the second holding frame J, F = max(0, C - target_zone_t). */
uint64_t ucfp_wang_stream_frontier(uint64_t n_samples, const ucfp_wang_config* cfg);
/* Host-only, no GPU: S(n) of A21, the final 8 kHz samples of a stream after n_samples input samples at sample_rate --
 * n at 8000; otherwise S(0) = 0 and S(n) = min(ceil((n - 1) 8000 / sr), floor(n 8000 / sr)): the outputs whose right
 * neighbour has arrived, capped at the offline length.  final != 0: floor(n 8000 / sr), the offline length.  0 for a
 * rate outside [1000, 384000].  The frontier of such a stream is ucfp_wang_stream_frontier(S, cfg) (Panako:
 * ucfp_panako_stream_frontier(S, cfg)). */
uint64_t ucfp_wang_stream_samples(uint64_t n_samples, uint32_t sample_rate, int final);
/* Host-only: device bytes a set holds per stream (0 for an out-of-range config). */
size_t ucfp_wang_streams_state_bytes(const ucfp_wang_config* cfg);
/* Host-only: the same with the ring of a window (A20; the reference has no audio matcher): state_bytes(cfg), plus
 * (window_frames != 0) 8 bytes of ring header and 8 bytes per window hash.  0 for out-of-range arguments. */
size_t ucfp_wang_streams_state_bytes_ex(const ucfp_wang_config* cfg, uint32_t window_frames);
/* Host-only: the same for a set of ucfp_wang_streams_create_sr (A21): state_bytes_ex(cfg, window_frames), plus
 * 4 * (ceil(sample_rate / 8000) + 1) bytes of carried input for sample_rate != 8000.  0 for out-of-range arguments. */
size_t ucfp_wang_streams_state_bytes_sr(const ucfp_wang_config* cfg, uint32_t window_frames, uint32_t sample_rate);
/* Host-only: hashes one stream's window can hold (A20; the reference has no audio matcher); 0 for window_frames = 0 or
 * out-of-range arguments. */
size_t ucfp_wang_streams_window_cap(const ucfp_wang_config* cfg, uint32_t window_frames);
/* Upper bound on the hashes a push can emit; host-computable from the per-slot sample counts (0 for an invalid push). */
size_t ucfp_wang_streams_max_hashes(ucfp_wang_streams* s, const uint32_t* slots, const uint64_t* n_samples,
                                    const uint8_t* final, size_t n);
/* slots / n_samples / final: host arrays of n entries (distinct open slots; final may be NULL = none); d_pcm: the n
 * chunks concatenated in that order on the device.  Hashes of entry i -> d_out[d_out_offsets[i] .. d_out_offsets[i+1])
 * (8 B each, t_anchor since the stream was opened; n + 1 device u64 offsets).  final[i] != 0 emits the rest and closes
 * the slot.  cap_hashes below ucfp_wang_streams_max_hashes -> UCFP_E_INVALID before ANY state changes.  One launch
 * sequence whatever n is; no host synchronisation (the host waits only for the table copy of the push two back). */
int ucfp_wang_streams_push_dev(ucfp_wang_streams* s, const uint32_t* slots, const uint64_t* n_samples,
                               const uint8_t* final, size_t n, const float* d_pcm, uint8_t* d_out, size_t cap_hashes,
                               uint64_t* d_out_offsets, void* stream);
/* Host-pointer convenience for one slot (the per-request shape of the reference route, handlers.rs:957-1010);
 * synchronous.  *n_hashes = hashes of this push. */
int ucfp_wang_streams_push(ucfp_wang_streams* s, uint32_t slot, const float* pcm, size_t n, int final, uint8_t* out,
                           size_t cap_hashes, size_t* n_hashes);
/* The live windows of n distinct open slots (A20; the hashes are those of StreamingWangSession::push, audio.rs:413-480,
 * the window itself has no counterpart: the reference has no audio matcher).  Item i = d_landmarks[d_offsets[i] ..
 * d_offsets[i+1]) with BYTE offsets (multiples of 8, n + 1 device u64) -- the query shape of
 * ucfp_landmark_index_query_dev -- and d_origins[i] = w0 (device u32, may be NULL).  d_landmarks must be 8-byte aligned.
 * cap_landmarks (8-byte hashes d_landmarks holds) below n * ucfp_wang_streams_window_cap -> UCFP_E_INVALID, as a closed
 * slot, a slot out of range or named twice, and a set created with window_frames = 0.  No host synchronisation. */
int ucfp_wang_streams_windows_dev(ucfp_wang_streams* s, const uint32_t* slots, size_t n, uint8_t* d_landmarks,
                                  size_t cap_landmarks, uint64_t* d_offsets, uint32_t* d_origins, void* stream);

/* STREAMING Panako (the reference has no streaming Panako): the stream set above with triplets behind
 * the same front end, plus a LIVE WINDOW per stream for ucfp_panako_index_query*.  A slot is one stream at 8 kHz.  After
 * a push that brings a stream to n samples the records emitted so far are exactly the offline records
 * (ucfp_audio_panako on the same samples) with t_a < F(n) (ucfp_panako_stream_frontier: A9's rule with the Panako
 * target_zone_t), in offline order; a final push emits the rest.  The concatenation over all pushes equals
 * ucfp_audio_panako of the whole stream byte for byte, however the stream is cut into chunks.  t_a, t_b, t_c count
 * frames since the stream was opened (u32; the 2^23-frame limit of one offline clip does not apply).
 *   - window_frames = W (0 .. UCFP_PANAKO_STREAM_MAX_WINDOW_FRAMES; 0 = no windows).  The window of an open stream at n
 *     samples is its emitted records with t_a >= w0 = max(0, F(n) - W), in emission order, with w0 subtracted from
 *     t_a, t_b and t_c (a query's t_a must stay below 2^28); at most ucfp_panako_streams_window_cap(cfg, W) =
 *     (ceil(2 W / 125) + 1) * peaks_per_sec * fan_out records.  Nothing emitted yet, a final push or close: empty.
 *     A hit's `offset` then says where stream frame w0 lies in the matched record.
 *   - Device bytes per stream: ucfp_panako_streams_state_bytes(cfg, W) = the Wang state for this config, plus (W != 0)
 *     8 bytes of ring header and 16 bytes per window record.
 *   - Serialisation, errors and "a failed call changes no state" as the Wang set; W above the maximum, a misaligned
 *     record buffer, a window call on a set without windows: UCFP_E_INVALID. */
typedef struct ucfp_panako_streams ucfp_panako_streams;
#define UCFP_PANAKO_STREAM_MAX_WINDOW_FRAMES 8192u /* 131 s */
/* sample_rate must be 8000, cfg inside the ranges of ucfp_panako_config (NULL = defaults): UCFP_E_MODALITY otherwise,
 * checked before anything else. */
int ucfp_panako_streams_create(ucfp_ctx* ctx, uint32_t sample_rate, const ucfp_panako_config* cfg, uint32_t max_streams,
                               uint32_t window_frames, ucfp_panako_streams** out);
/* As ucfp_wang_streams_create_sr (A21): a feed at any rate from 1 000 to 384 000 Hz, resampled on the device; the
 * concatenation over all pushes equals ucfp_audio_panako_batch_dev over the one clip at that rate byte for byte.
 * n_samples count input samples, S(n) = ucfp_wang_stream_samples; times and W stay in 8 kHz frames.  At 8000 this is
 * ucfp_panako_streams_create exactly. */
int ucfp_panako_streams_create_sr(ucfp_ctx* ctx, uint32_t sample_rate, const ucfp_panako_config* cfg,
                                  uint32_t max_streams, uint32_t window_frames, ucfp_panako_streams** out);
void ucfp_panako_streams_destroy(ucfp_panako_streams* s);
int ucfp_panako_streams_open(ucfp_panako_streams* s, uint32_t* slot);     /* fresh stream, t = 0, empty window */
int ucfp_panako_streams_close(ucfp_panako_streams* s, uint32_t slot);     /* discard, emit nothing */
/* Host-only, no GPU: F(n) as ucfp_wang_stream_frontier, with the Panako target_zone_t. */
uint64_t ucfp_panako_stream_frontier(uint64_t n_samples, const ucfp_panako_config* cfg);
/* Host-only: device bytes a set holds per stream (0 for an out-of-range config or window). */
size_t ucfp_panako_streams_state_bytes(const ucfp_panako_config* cfg, uint32_t window_frames);
/* Host-only: the same for a set of ucfp_panako_streams_create_sr (A21): plus 4 * (ceil(sample_rate / 8000) + 1) bytes
 * of carried input for sample_rate != 8000.  0 for out-of-range arguments. */
size_t ucfp_panako_streams_state_bytes_sr(const ucfp_panako_config* cfg, uint32_t window_frames, uint32_t sample_rate);
/* Host-only: records one stream's window can hold (0 for window_frames = 0 or out-of-range arguments). */
size_t ucfp_panako_streams_window_cap(const ucfp_panako_config* cfg, uint32_t window_frames);
/* Upper bound on the records a push can emit (0 for an invalid push). */
size_t ucfp_panako_streams_max_hashes(ucfp_panako_streams* s, const uint32_t* slots, const uint64_t* n_samples,
                                      const uint8_t* final, size_t n);
/* As ucfp_wang_streams_push_dev; records of entry i -> d_out[d_out_offsets[i] .. d_out_offsets[i+1]) in RECORDS (16 B
 * each; n + 1 device u64).  d_out must be 16-byte aligned.  cap_hashes below ucfp_panako_streams_max_hashes ->
 * UCFP_E_INVALID before ANY state changes.  No host synchronisation. */
int ucfp_panako_streams_push_dev(ucfp_panako_streams* s, const uint32_t* slots, const uint64_t* n_samples,
                                 const uint8_t* final, size_t n, const float* d_pcm, uint8_t* d_out, size_t cap_hashes,
                                 uint64_t* d_out_offsets, void* stream);
/* Host-pointer convenience for one slot; synchronous.  *n_hashes = records of this push. */
int ucfp_panako_streams_push(ucfp_panako_streams* s, uint32_t slot, const float* pcm, size_t n, int final, uint8_t* out,
                             size_t cap_hashes, size_t* n_hashes);
/* The live windows of n distinct open slots: item i = d_records[d_offsets[i] .. d_offsets[i+1]) with BYTE offsets
 * (multiples of 16, n + 1 device u64) -- the query shape of ucfp_panako_index_query_dev -- and d_origins[i] = w0 (device
 * u32, may be NULL).  cap_records (16-byte records d_records holds) below n * ucfp_panako_streams_window_cap ->
 * UCFP_E_INVALID.  No host synchronisation. */
int ucfp_panako_streams_windows_dev(ucfp_panako_streams* s, const uint32_t* slots, size_t n, uint8_t* d_records,
                                    size_t cap_records, uint64_t* d_offsets, uint32_t* d_origins, void* stream);

size_t ucfp_audio_haitsma_frames(size_t n_samples, uint32_t sample_rate);
int ucfp_audio_haitsma(ucfp_ctx* ctx, const float* pcm, size_t n, uint32_t sample_rate,
                       const ucfp_haitsma_config* cfg, uint32_t* out, size_t cap_frames, size_t* n_frames);
/* Device buffers; the input must already be at 5 kHz (use ucfp_audio_resample_linear_dev). */
int ucfp_audio_haitsma_dev(ucfp_ctx* ctx, const float* d_pcm5k, size_t n, const ucfp_haitsma_config* cfg,
                           uint32_t* d_out, size_t cap_frames, void* stream);

/* RAGGED BATCH for Haitsma, same shape as ucfp_audio_wang_batch_dev: clip i = d_pcm[d_offsets[i] .. d_offsets[i+1]) at
 * `sample_rate`; clips at another rate than 5 kHz are resampled (A1) into the context's workspace first, like
 * audio.rs:194-200 does per clip.  Sub-fingerprints of clip i land in d_out[d_out_offsets[i] .. d_out_offsets[i+1])
 * (u32 each; a clip's first frame has a zero history); frames past cap_frames are not written (d_out_offsets[n_clips]
 * tells).  One launch sequence for the whole batch. */
size_t ucfp_audio_haitsma_batch_max_frames(size_t n_total, size_t n_clips, uint32_t sample_rate);
int ucfp_audio_haitsma_batch_dev(ucfp_ctx* ctx, const float* d_pcm, const uint64_t* d_offsets, size_t n_total, size_t n_clips,
                                 uint32_t sample_rate, const ucfp_haitsma_config* cfg, uint32_t* d_out, size_t cap_frames,
                                 uint64_t* d_out_offsets, void* stream);

/* audiofp::dsp::resample::linear. Output length = floor(n * sr_out / sr_in). */
size_t ucfp_audio_resample_len(size_t n, uint32_t sr_in, uint32_t sr_out);
int ucfp_audio_resample_linear_dev(ucfp_ctx* ctx, const float* d_in, size_t n, uint32_t sr_in, uint32_t sr_out,
                                   float* d_out, size_t cap, void* stream);

/* =============================== TEXT =========================================
 * Replaces the arithmetic behind
 *   text::fingerprint_minhash_with::<128>   src/modality/text.rs:182-236  (1032-B MinHashSig<128>)
 *   text::fingerprint_simhash_tf / _idf     src/modality/text.rs:328-421  (8-B SimHash64)
 *   text::fingerprint_lsh                   src/modality/text.rs:437-446  (same bytes as minhash)
 * i.e. txtfp::MinHashFingerprinter / SimHashFingerprinter.  Documents are passed as one UTF-8
 * blob plus n+1 byte offsets.
 *   UCFP_TEXT_RAW_ASCII     the GPU canonicalises (ASCII lower-casing; NFKC / case fold / Cf+Bidi
 *                           stripping are the identity on ASCII) and segments (UAX#29 restricted
 *                           to ASCII).  A document holding a byte >= 0x80 gets status
 *                           UCFP_TEXT_NEEDS_HOST: the host canonicalises + tokenises it
 *                           (Unicode tables live there) and resubmits it as
 *   UCFP_TEXT_PRETOKENIZED  tokens already canonical, separated by single spaces.  Every byte other
 *                           than ' ' is a token byte, 0x00 included.
 *   UCFP_TEXT_RAW_UTF8      the GPU canonicalises (NFKC + case fold + Cf stripping, text.rs:112-114, as a table of
 *                           per-code-point mappings) and segments (UAX#29 words as the host path finds them) any
 *                           UTF-8 document over the COVERED set of code points (ASCII, Latin, Greek,
 *                           Cyrillic, Hebrew, Arabic, punctuation, kana, Han, Hangul syllables, compatibility forms;
 *                           include/ucfp_text_utab.h), then hashes the result as PRETOKENIZED.  The record is the one
 *                           the host path (canonicalise + tokenise on the host, PRETOKENIZED) gives.  A document with
 *                           malformed UTF-8 or an uncovered code point (combining marks, Hangul jamo, regional
 *                           indicators, unassigned ...) gets UCFP_TEXT_NEEDS_HOST and a zero record; that status wins
 *                           over the hash pass's.  Unlike RAW_ASCII this mode follows UAX#29 for '_' and has the
 *                           `regex` module's apostrophe tailoring, so an ASCII document gives the same record in both
 *                           modes iff it holds neither '_' nor '\''.  The _dev calls read d_offsets[0] and
 *                           d_offsets[n] back (they wait for `stream` once) to size the context's scratch.
 * status[i]: 0, UCFP_TEXT_NEEDS_HOST, UCFP_E_MODALITY (no tokens), UCFP_E_UNSUPPORTED (k - 1 tokens
 * plus the token being read do not fit the LDS batch, see UCFP_TEXT_MAX_WINDOW_BYTES).
 */
#define UCFP_TEXT_RAW_ASCII 0
#define UCFP_TEXT_PRETOKENIZED 1
#define UCFP_TEXT_RAW_UTF8 2
#define UCFP_TEXT_NEEDS_HOST 1
/* A document is ALWAYS hashed (never UCFP_E_UNSUPPORTED) when every window of k consecutive tokens -- the whole
 * document when it has fewer than k tokens, the single token for SimHash -- has a canonical length (token bytes plus
 * the k - 1 separating spaces) of at most this many bytes.  Longer windows are hashed or refused depending on where
 * the 64-byte steps fall; a window longer than the 1536-byte batch is always refused.  A refused document's record is
 * all zero.
 * Derivation (text.hip): a wave keeps the canonical stream of the current batch in kCanonCap = 1536 bytes of LDS.
 * Before each 64-byte step it demands room for the step, `cbase + ntok + 130 <= kCanonCap`, where cbase + ntok is the
 * canonical length in use plus 1 (cbase token bytes, ntok - 1 separators).  When that fails the batch is flushed:
 * everything is consumed except the last k - 1 complete tokens and the unfinished token, i.e. a PREFIX of one k-token
 * window, which moves to the front.  The document is refused exactly when the check fails again right after a flush
 * (or the flush could consume nothing because fewer than k tokens are complete -- the batch is then itself such a
 * prefix): prefix + 1 + 130 > 1536, i.e. prefix >= 1406.  A prefix is no longer than its window, so windows of at
 * most 1536 - 130 - 1 = 1405 bytes are never refused.  (The token cap, ntok + 33 <= 256, cannot fail after a flush:
 * at most k <= 64 tokens are kept.) */
#define UCFP_TEXT_MAX_WINDOW_BYTES 1405
#define UCFP_MINHASH_BYTES 1032 /* txtfp::MinHashSig<128>: u16 schema = 1, 6 pad, 128 x u64 LE */
/* COMPATIBILITY: the LAYOUT is txtfp's, the 128 slot VALUES are not -- txtfp 0.2.0's slot derivation could not be
 * recovered offline (the reference's golden slot 0, src/server/tests.rs:1153-1157, is not
 * reproduced).  Records made here must therefore never be compared with upstream `minhash-h128` records: the host
 * stores them with format_version UCFP_MINHASH_FORMAT_VERSION instead of txtfp::FORMAT_VERSION (text.rs:227), so a
 * mixed corpus is rejected as incompatible rather than yielding meaningless Jaccard estimates.  SimHash (XXH3-64 per
 * token, family pinned by tests.rs:1126-1127) carries txtfp's own format_version. */
#define UCFP_MINHASH_FORMAT_VERSION 0x48500001u
#define UCFP_SIMHASH_BYTES 8

int ucfp_text_minhash_batch_dev(ucfp_ctx* ctx, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n,
                                int mode, uint32_t shingle_k, uint8_t* d_out, int32_t* d_status, void* stream);
int ucfp_text_minhash_batch(ucfp_ctx* ctx, const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode,
                            uint32_t shingle_k, uint8_t* out, int32_t* status);
int ucfp_text_simhash_batch_dev(ucfp_ctx* ctx, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n,
                                int mode, uint8_t* d_out, int32_t* d_status, void* stream);
int ucfp_text_simhash_batch(ucfp_ctx* ctx, const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode,
                            uint8_t* out, int32_t* status);

/* TOKENISERS.  Every text request of the reference names a tokeniser (src/server/dto.rs,
 * handlers.rs:532-539; text.rs:66-83): MinHash wraps it in ShingleTokenizer { k, inner } (text.rs:194-219), SimHash is fed
 * its raw tokens (text.rs:379-398).  The _ex entries take it as a parameter:
 *   UCFP_TEXT_TOK_WORD      the entries above, unchanged (every mode).
 *   UCFP_TEXT_TOK_GRAPHEME  the tokens are the UAX#29 extended grapheme clusters of the canonical text, as the host finds
 *                           them with `regex.findall(r"\X", canon)`; EVERY cluster is a token, whitespace, punctuation
 *                           and controls included.  Modes:
 *     UCFP_TEXT_RAW_ASCII   canonical text = the bytes with A-Z lower-cased, every byte kept (0x00 too); a cluster is one
 *                           byte, CR LF one cluster.  A byte >= 0x80 gives UCFP_TEXT_NEEDS_HOST.  One launch.
 *     UCFP_TEXT_RAW_UTF8    canonical text = the concatenation of M(c) (U2, U3: strict decode, NFKC + case fold + Cf
 *                           stripping as a table); a cluster is one canonical code point, CR LF one cluster.  That holds
 *                           over the GRAPHEME SET (G3): the code points U1 covers, less those with a code point of M(c)
 *                           whose Grapheme_Cluster_Break is Prepend, L, V or T (twelve Prepend letters, the Hangul jamo
 *                           U1 keeps; include/ucfp_text_gtab.h; ucfp_text_grapheme_covered).  A document with another
 *                           code point or malformed UTF-8 gets UCFP_TEXT_NEEDS_HOST and a zero record, and that status
 *                           wins; the host cuts its clusters and submits them to the token entries below.  An ASCII
 *                           document gives the same record in both modes.  The _dev calls read d_offsets[0] and
 *                           d_offsets[n] back once, as the word route's do.
 *     UCFP_TEXT_PRETOKENIZED  UCFP_E_INVALID: a cluster may be or hold a space; tokens go to the token entries.
 *   Shingles, hashes, records, statuses, shingle_k's range and the alignment of the outputs are those of the entries above
 *   (k consecutive tokens joined by one 0x20; fewer than k tokens in the document: one shingle of all of them; none:
 *   UCFP_E_MODALITY).  An unknown tokeniser or mode gives UCFP_E_INVALID.
 * CALLER-SEGMENTED TOKENS: the route for any tokeniser the host runs itself (grapheme hand-backs, Lindera's cjk-jp /
 * cjk-ko tokens).  Token t is bytes[tok_offsets[t], tok_offsets[t + 1]), any byte string, 0x20 and 0x00 included, hashed
 * as it is; an empty token is not a token.  Document i owns the tokens doc_tokens[i] .. doc_tokens[i + 1] - 1; tok_offsets
 * has doc_tokens[n] + 1 entries.  For tokens that hold no 0x20 the record and status are those of the PRETOKENIZED entries
 * over the tokens joined by single spaces, byte for byte.
 *   - The host entries check both tables whole before anything runs (ucfp_text_tokens_validate: non-decreasing, which
 *     keeps every token inside [tok_offsets[doc_tokens[0]], tok_offsets[doc_tokens[n]])); otherwise UCFP_E_INVALID.
 *   - The _dev entries cannot: there the wave of a document checks its own slice before it reads a byte of the blob.  A
 *     document with a decreasing pair of offsets, or with a range outside the announced one (tokens doc_tokens[0] ..
 *     doc_tokens[n], bytes between those two tokens' offsets), gets status UCFP_E_INVALID and a zero record; the others
 *     are hashed.  No byte outside the announced range is read.  Nothing is read back and no scratch is used.
 * WINDOW LIMIT: UCFP_TEXT_MAX_WINDOW_BYTES holds for all of these entries as stated above.  A step of these kernels can open
 * 64 tokens and add 64 separators where the word step opens 32; the room a step demands (130 bytes) covers 64 + 64, and
 * the token cap is checked against 64 (ntok + 64 <= 256), which cannot fail after a flush either: at most k <= 64 tokens
 * are kept (text_core.h pins both with static_asserts). */
#define UCFP_TEXT_TOK_WORD 0
#define UCFP_TEXT_TOK_GRAPHEME 1
/* text.rs:194-219 with `inner` = the tokeniser named by `tokenizer` (text.rs:66-83); handlers.rs:532-539 */
int ucfp_text_minhash_batch_ex_dev(ucfp_ctx* ctx, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, int mode,
                                   int tokenizer, uint32_t shingle_k, uint8_t* d_out, int32_t* d_status, void* stream);
int ucfp_text_minhash_batch_ex(ucfp_ctx* ctx, const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode, int tokenizer,
                               uint32_t shingle_k, uint8_t* out, int32_t* status);
/* text.rs:379-398 (raw tokens of the tokeniser named by `tokenizer`, no shingling); handlers.rs:532-539 */
int ucfp_text_simhash_batch_ex_dev(ucfp_ctx* ctx, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, int mode,
                                   int tokenizer, uint8_t* d_out, int32_t* d_status, void* stream);
int ucfp_text_simhash_batch_ex(ucfp_ctx* ctx, const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode, int tokenizer,
                               uint8_t* out, int32_t* status);
/* text.rs:194-219 behind a tokeniser the host ran (text.rs:66-83: cjk-jp, cjk-ko; grapheme hand-backs) */
int ucfp_text_minhash_tokens_batch_dev(ucfp_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_tok_offsets,
                                       const uint64_t* d_doc_tokens, size_t n, uint32_t shingle_k, uint8_t* d_out,
                                       int32_t* d_status, void* stream);
int ucfp_text_minhash_tokens_batch(ucfp_ctx* ctx, const uint8_t* bytes, const uint64_t* tok_offsets, const uint64_t* doc_tokens,
                                   size_t n, uint32_t shingle_k, uint8_t* out, int32_t* status);
/* text.rs:379-398 behind a tokeniser the host ran */
int ucfp_text_simhash_tokens_batch_dev(ucfp_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_tok_offsets,
                                       const uint64_t* d_doc_tokens, size_t n, uint8_t* d_out, int32_t* d_status, void* stream);
int ucfp_text_simhash_tokens_batch(ucfp_ctx* ctx, const uint8_t* bytes, const uint64_t* tok_offsets, const uint64_t* doc_tokens,
                                   size_t n, uint8_t* out, int32_t* status);

/* MINHASH WITH ANY SLOT COUNT.  The reference's entry point is generic over the slot count,
 * fingerprint_minhash_with::<const H> (src/modality/text.rs:182-236); its manifest offers h from 16 to 1024 in steps of 16
 * and the presets (k = 3, h = 256) and (k = 7, h = 64) (src/server/algorithms_manifest.rs:280-328).
 *   h        a multiple of UCFP_MINHASH_H_STEP in [UCFP_MINHASH_H_MIN, UCFP_MINHASH_H_MAX]; anything else UCFP_E_INVALID
 *   record   UCFP_MINHASH_RECORD_BYTES(h) = 8 + 8 h bytes: u16 LE schema = 1, six zero bytes, h u64 LE slots;
 *            slot i = min over the document's shingles of h1 + i * h2 mod 2^64 (T5 continued to i < h), so the slots of
 *            h' < h are the first h' slots of h over the same text
 *   out      rows 8 + 8 h bytes apart, 4-byte alignment; a document whose status is not 0 gets a zero record
 * Modes, tokenisers, statuses, shingle_k's range, UCFP_TEXT_MAX_WINDOW_BYTES and the validation order are those of the _ex
 * and token entries above; h is checked after the tokeniser.  h = 128 writes what those entries write, byte for byte.
 * COMPATIBILITY as for UCFP_MINHASH_BYTES: layout txtfp's, slot values ours (UCFP_MINHASH_FORMAT_VERSION). */
#define UCFP_MINHASH_H_MIN 16
#define UCFP_MINHASH_H_MAX 1024
#define UCFP_MINHASH_H_STEP 16
#define UCFP_MINHASH_RECORD_BYTES(h) (8 + 8 * (size_t)(h))
/* text.rs:182-236 (fingerprint_minhash_with::<H>) behind the tokeniser named by `tokenizer` */
int ucfp_text_minhash_h_batch_dev(ucfp_ctx* ctx, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, int mode, int tokenizer,
                                  uint32_t shingle_k, uint32_t h, uint8_t* d_out, int32_t* d_status, void* stream);
int ucfp_text_minhash_h_batch(ucfp_ctx* ctx, const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode, int tokenizer,
                              uint32_t shingle_k, uint32_t h, uint8_t* out, int32_t* status);
/* text.rs:182-236 behind a tokeniser the host ran */
int ucfp_text_minhash_tokens_h_batch_dev(ucfp_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_tok_offsets,
                                         const uint64_t* d_doc_tokens, size_t n, uint32_t shingle_k, uint32_t h, uint8_t* d_out,
                                         int32_t* d_status, void* stream);
int ucfp_text_minhash_tokens_h_batch(ucfp_ctx* ctx, const uint8_t* bytes, const uint64_t* tok_offsets, const uint64_t* doc_tokens,
                                     size_t n, uint32_t shingle_k, uint32_t h, uint8_t* out, int32_t* status);
/* Host-only (no device, no context): 1 iff the grapheme set (G3) covers cp.  text.rs:66-83 (Grapheme). */
int ucfp_text_grapheme_covered(uint32_t cp);
/* Host-only: the check the host token entries make of their tables -- doc_tokens[0 .. n] and tok_offsets[doc_tokens[0] ..
 * doc_tokens[n]] non-decreasing.  UCFP_OK or UCFP_E_INVALID.  text.rs:194-219 (the tokens of one document are a sequence). */
int ucfp_text_tokens_validate(const uint64_t* tok_offsets, const uint64_t* doc_tokens, size_t n);

/* IDF: text::fingerprint_simhash_idf(text, opts, &IdfTable, ..) (src/modality/text.rs:344-362) with a table
 * the caller supplies (the reference's own use; dto.rs:489-493 names server-side tables) or fits to a corpus on the GPU.
 * txtfp's IdfTable and Weighting::IdfWeighted arithmetic are in a crate that is not available: every rule below is this
 * library's own and "bit-exact" means against tests/simhash_idf_ref.py.
 *   KEY (T9.1)      XXH3_64(canonical token bytes, seed 0), the value TF SimHash hashes: one table serves every tokeniser
 *                   and input form.  Every u64 is a legal key, 0 and 2^64 - 1 included.
 *   WEIGHT (T9.2)   u32 in Q16.16 (0x10000 = 1.0); all sums are 64-bit integers, so a record depends on neither the order of
 *                   the tokens nor the device.  0 is legal and removes the token (a stop word).
 *   RECORD (T9.3)   every token occurrence adds w(t) -- the table's weight of its key, else the table's default -- to tot,
 *                   and to pos_b for every set bit b of its key; bit b of the record is set iff 2 pos_b > tot (a tie clears
 *                   it).  Equal non-zero weights give the TF record.  Statuses are those of the TF entry over the same
 *                   input, plus UCFP_E_MODALITY (-1) and a zero record for a document whose tot is 0.
 *   FIT (T9.4)      a table counts N, the documents added with status 0, and per key df, those of them that hold the key
 *                   at least once.  finalize gives weight(df) = 0x10000 + L(N + 1) - L(df + 1) and default = weight(0),
 *                   L = ucfp_idf_log2_q16, an integer log2 in Q16 within (-1, 0] units of 65536 log2(x) (base 2 instead
 *                   of ln only rescales the IDF term against the + 1).  A document with any other status adds nothing.
 *   SUPPLIED (T9.5) set_weights REPLACES the table's contents by the given (key, weight) pairs and default and marks it
 *                   final; N and every df are then 0.  A key given twice: UCFP_E_INVALID and nothing changes.
 *   LIFECYCLE (T9.6) an add after finalize / set_weights makes the table not final; the weighted SimHash entries give
 *                   UCFP_E_INVALID for a table that is not final; finalize of an empty table is legal (every token weighs
 *                   1.0: TF records).  One thread mutates a table at a time; any number may read a final one.  finalize
 *                   runs on `stream`, waits for it and frees the table's fit scratch: the weights are written when it
 *                   returns.
 *   TABLE           open addressing in device memory, at most half full (it grows by rehashing into twice the size or more
 *                   before the inserts that need the room, behind a synchronisation of the stream: a fit step).
 *   ADD             the forms, argument checks and statuses of ucfp_text_simhash_batch_ex / _simhash_tokens_batch.  The
 *                   batch is worked off in pieces of at most piece_tokens slots (0: 2^22; a document owns one slot per byte
 *                   -- per announced token in the token form -- and a larger document is a piece of its own); the scratch
 *                   (12 bytes per slot, twice, plus the sort's) belongs to the table.  The _dev forms read d_offsets /
 *                   d_doc_tokens back to plan the pieces and synchronise `stream` per piece; a decreasing doc_tokens is
 *                   refused whole (UCFP_E_INVALID), tok_offsets is checked per document on the device as in the TF entry.
 *                   d_status may be NULL.
 *   EXPORT          unordered (key, df, weight) triples; weights are meaningful once the table is final.  With cap = 0 and
 *                   NULL arrays it only reports *n and *default_q16; cap < *n otherwise is UCFP_E_INVALID. */
typedef struct ucfp_idf_table ucfp_idf_table;
/* text.rs:344-362 (the IdfTable argument) */
int ucfp_idf_table_create(ucfp_ctx* ctx, size_t capacity_hint, size_t piece_tokens, uint32_t flags, ucfp_idf_table** out);
void ucfp_idf_table_destroy(ucfp_idf_table* t);
/* text.rs:344-362: the corpus side of the table, tokens as ucfp_text_simhash_batch_ex cuts them */
int ucfp_idf_table_add_batch_dev(ucfp_idf_table* t, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, int mode,
                                 int tokenizer, int32_t* d_status, void* stream);
int ucfp_idf_table_add_batch(ucfp_idf_table* t, const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode, int tokenizer,
                             int32_t* status);
/* text.rs:344-362: the same behind a tokeniser the host ran */
int ucfp_idf_table_add_tokens_batch_dev(ucfp_idf_table* t, const uint8_t* d_bytes, const uint64_t* d_tok_offsets,
                                        const uint64_t* d_doc_tokens, size_t n, int32_t* d_status, void* stream);
int ucfp_idf_table_add_tokens_batch(ucfp_idf_table* t, const uint8_t* bytes, const uint64_t* tok_offsets,
                                    const uint64_t* doc_tokens, size_t n, int32_t* status);
/* text.rs:344-362: a caller-made table */
int ucfp_idf_table_set_weights(ucfp_idf_table* t, const uint64_t* keys, const uint32_t* weights_q16, size_t n,
                               uint32_t default_q16);
int ucfp_idf_table_finalize(ucfp_idf_table* t, void* stream);
int ucfp_idf_table_size(ucfp_idf_table* t, uint64_t* n_docs, size_t* n_keys, int* is_final);
int ucfp_idf_table_export(ucfp_idf_table* t, uint64_t* keys, uint32_t* dfs, uint32_t* weights_q16, size_t cap, size_t* n,
                          uint32_t* default_q16);
/* Host-only (no device, no context): T9.4's L and weight(df), T9.1's key.  text.rs:344-362. */
uint32_t ucfp_idf_log2_q16(uint64_t x);
uint32_t ucfp_idf_weight_q16(uint64_t n_docs, uint64_t df);
uint64_t ucfp_text_token_key(const uint8_t* bytes, size_t len);
/* text.rs:344-362: the weighted record; forms of ucfp_text_simhash_batch_ex and ucfp_text_simhash_tokens_batch */
int ucfp_text_simhash_idf_batch_dev(ucfp_ctx* ctx, const ucfp_idf_table* table, const uint8_t* d_utf8, const uint64_t* d_offsets,
                                    size_t n, int mode, int tokenizer, uint8_t* d_out, int32_t* d_status, void* stream);
int ucfp_text_simhash_idf_batch(ucfp_ctx* ctx, const ucfp_idf_table* table, const uint8_t* utf8, const uint64_t* offsets, size_t n,
                                int mode, int tokenizer, uint8_t* out, int32_t* status);
int ucfp_text_simhash_idf_tokens_batch_dev(ucfp_ctx* ctx, const ucfp_idf_table* table, const uint8_t* d_bytes,
                                           const uint64_t* d_tok_offsets, const uint64_t* d_doc_tokens, size_t n, uint8_t* d_out,
                                           int32_t* d_status, void* stream);
int ucfp_text_simhash_idf_tokens_batch(ucfp_ctx* ctx, const ucfp_idf_table* table, const uint8_t* bytes,
                                       const uint64_t* tok_offsets, const uint64_t* doc_tokens, size_t n, uint8_t* out,
                                       int32_t* status);

/* STREAMING MinHash: text::StreamingMinHashSession::new / push / finalize (src/modality/text.rs:645-730)
 * behind POST /v1/ingest/text/{tid}/{rid}/stream (src/server/handlers.rs:590-626), with the state on the device and many
 * streams advanced by one push.  The reference buffers the document and hashes it at the end; here a stream keeps the 128
 * running minima, the last k - 1 complete tokens, the unfinished token and one held-back byte on the device
 * (ucfp_text_streams_state_bytes, about 3 KiB), whatever its length.  A set holds max_streams slots.
 * CONTRACT.  Let B be the concatenation of a stream's chunks, however they are cut.  The final record and status equal
 * those of ucfp_text_minhash_batch(mode, shingle_k) on the one document B, byte for byte, whenever every k-token window
 * of B has at most UCFP_TEXT_MAX_WINDOW_BYTES canonical bytes.  The derivation is the offline one: the state carried
 * from push to push is what the offline kernel keeps over a flush, a prefix of one window, so the room check cannot
 * fail twice in a row.  Above that limit a stream promises what the offline path promises: either status 0 with the
 * exact record, or a zero record with a nonzero status -- always the latter above 1536 bytes.
 *   - The last byte of a non-final push is held back and processed by the next one: whether a byte is inside a word
 *     depends on the byte after it (offline, the byte past the end reads as 0; a stream does not guess it).
 *   - d_status[i] is the stream's status after the push: 0; UCFP_TEXT_NEEDS_HOST (a byte >= 0x80 was seen in a
 *     RAW_ASCII stream, the held-back byte included); UCFP_E_UNSUPPORTED (the window limit was hit); UCFP_E_MODALITY
 *     (no tokens: only on a final entry).  NEEDS_HOST and UCFP_E_UNSUPPORTED are sticky: later pushes are accepted and
 *     change nothing, the final record is all zero with that status.
 *   - The set serialises its own calls: it is safe to call from several threads.  Consecutive pushes are ordered by
 *     the set itself (an event), whatever `stream` the caller passes.  ucfp_text_streams_push_dev allocates nothing.
 *   - One wave works on one chunk, so a long chunk is serial on that wave: cut long documents into several pushes
 *     only if latency matters, the record does not depend on it.
 *   - A failed call changes no state.
 * UTF-8 STREAMS (a set created by ucfp_text_streams_create_ex with UCFP_TEXT_STREAMS_UTF8 also opens streams in mode
 * UCFP_TEXT_RAW_UTF8).  The contract above holds for them, with the window limit counted in CANONICAL bytes and one
 * more condition, on open segments, below.  A push stays ONE launch: the wave of an entry canonicalises its chunk into
 * scratch the set owns (sized at creation from max_push_bytes) and hashes the canonical bytes as the next piece of a
 * PRETOKENIZED stream.  Chunks may be cut anywhere: inside a UTF-8 sequence, between a letter and the MidLetter after
 * it, inside a run of Cf characters.
 *   - The trailing bytes of a UTF-8 sequence a non-final chunk does not finish (at most 3) are held, raw, for the next
 *     chunk: no error.  A sequence still unfinished at the FINAL push is malformed.
 *   - The last canonical code point made so far stays undecided until its right neighbour arrives (the boundary before
 *     x[i] needs x[i + 1]); Cf code points make nothing, so a trailing run of them is consumed, not held.
 *     A final push decides everything and closes the open segment.
 *   - OPEN SEGMENT.  A segment is a token iff it holds an alphanumeric (U5).  The segment still open at the end of a
 *     non-final push is emitted so far if it already holds one; otherwise its canonical bytes (its separator included)
 *     wait in the slot's state, which has room for UCFP_TEXT_STREAM_OPEN_SEGMENT_BYTES.  THIS IS THE ONE PLACE WHERE A
 *     STREAM MAY REFUSE WHAT THE OFFLINE CALL HASHES: if more are pending at a push boundary -- 256 or more bytes of
 *     `_`, say, with no letter or digit yet -- the stream gets UCFP_TEXT_NEEDS_HOST.  Within one push any length is
 *     handled as offline.
 *   - UCFP_TEXT_NEEDS_HOST: an uncovered code point, malformed UTF-8 (U2's strict rules), or the open-segment
 *     condition.  Sticky, zero final record, never reported before the offending byte was pushed, and it wins over the
 *     hash stage's status, as offline.  UCFP_E_UNSUPPORTED and UCFP_E_MODALITY as above.
 *   - The RAW_UTF8 chunks of one push may have max_push_bytes bytes in all; a push above that fails with UCFP_E_INVALID
 *     and changes no state.  Per stream the set holds ucfp_text_streams_state_bytes_ex(UCFP_TEXT_STREAMS_UTF8) bytes. */
#define UCFP_TEXT_STREAMS_UTF8 1u
#define UCFP_TEXT_STREAM_OPEN_SEGMENT_BYTES 256u
typedef struct ucfp_text_streams ucfp_text_streams;
/* text.rs:645-730, handlers.rs:590-626.  shingle_k outside [1, 64] -> UCFP_E_MODALITY (as ucfp_text_minhash_batch), checked
 * before anything else; max_streams in [1, 2^20].  Fails with UCFP_E_INDEX without a gfx950 device (no CPU fallback). */
int ucfp_text_streams_create(ucfp_ctx* ctx, uint32_t shingle_k, uint32_t max_streams, ucfp_text_streams** out);
/* text.rs:645-730, handlers.rs:590-626, with txtfp's canonicaliser and tokeniser (text.rs:112-114,182-236) on the device for
 * the streams opened RAW_UTF8.  flags: 0 (= ucfp_text_streams_create; max_push_bytes is ignored) or
 * UCFP_TEXT_STREAMS_UTF8, then max_push_bytes in [1, 2^28]: the RAW_UTF8 chunk bytes one push may carry; the set
 * allocates 4 x that plus about 400 bytes per slot of scratch once, here.  Unknown flags -> UCFP_E_INVALID. */
int ucfp_text_streams_create_ex(ucfp_ctx* ctx, uint32_t shingle_k, uint32_t max_streams, uint32_t flags, uint64_t max_push_bytes,
                                ucfp_text_streams** out);
/* text.rs:645-730, handlers.rs:590-626 */
void ucfp_text_streams_destroy(ucfp_text_streams* s);
/* text.rs:645-730, handlers.rs:590-626.  A fresh stream in the first free slot.  mode: UCFP_TEXT_RAW_ASCII or
 * UCFP_TEXT_PRETOKENIZED; UCFP_TEXT_RAW_UTF8 on a set created with UCFP_TEXT_STREAMS_UTF8, on any other set
 * -> UCFP_E_UNSUPPORTED (the set has no streaming canonicaliser); any other value, or a full set -> UCFP_E_INVALID. */
int ucfp_text_streams_open(ucfp_text_streams* s, int mode, uint32_t* slot);
/* text.rs:645-730, handlers.rs:590-626.  Discard the stream, emit nothing. */
int ucfp_text_streams_close(ucfp_text_streams* s, uint32_t slot);
/* text.rs:645-730, handlers.rs:590-626.  Host-only: device bytes a set holds per stream. */
size_t ucfp_text_streams_state_bytes(void);
/* text.rs:645-730, handlers.rs:590-626.  Host-only: the same for a set created with `flags` (the canon stage's state on
 * top for UCFP_TEXT_STREAMS_UTF8: context, held bytes, the pending open segment). */
size_t ucfp_text_streams_state_bytes_ex(uint32_t flags);
/* text.rs:645-730, handlers.rs:590-626.  slots / n_bytes / final: host arrays of n entries (distinct open slots; final may
 * be NULL = none; a chunk of 0 bytes is legal, final or not); d_bytes: the n chunks concatenated in that order on the
 * device (any alignment).  d_out: n x 1032 bytes (n x ucfp_text_streams_record_bytes: 8 for a SimHash set), entry i is
 * written only when final[i] is set (NULL allowed when no entry is final); a final entry frees its slot.  d_status:
 * n x int32, see above.  UCFP_E_INVALID before ANY state changes: a slot out of range, not open or listed twice, a stream
 * that would pass 2^63 bytes (a SimHash stream: reach UCFP_TEXT_SIMHASH_STREAM_LIMIT_BYTES), RAW_UTF8 chunks of more than
 * the set's max_push_bytes in all, a SimHash set's table that is not final.  One launch whatever n is; no host
 * synchronisation (the host waits only for the table copy of the push two back). */
int ucfp_text_streams_push_dev(ucfp_text_streams* s, const uint32_t* slots, const uint64_t* n_bytes, const uint8_t* final,
                               size_t n, const uint8_t* d_bytes, uint8_t* d_out, int32_t* d_status, void* stream);
/* text.rs:645-730, handlers.rs:590-626.  Host-pointer convenience for one slot (the per-request shape of the reference
 * route); synchronous.  out (1032 bytes; ucfp_text_streams_record_bytes) may be NULL unless final is set; status may be NULL. */
int ucfp_text_streams_push(ucfp_text_streams* s, uint32_t slot, const uint8_t* bytes, size_t n, int final, uint8_t* out,
                           int32_t* status);

/* STREAMING SimHash: the other record a text request can ask for (text::fingerprint_simhash_tf,
 * src/modality/text.rs:328-343, and fingerprint_simhash_idf, text.rs:344-362, whose record body is text.rs:364-421)
 * behind the session shape of text.rs:645-730.  The reference has no such session; a set made by
 * ucfp_text_streams_create_sim is a ucfp_text_streams whose streams end in the 8-byte SimHash record instead of the
 * MinHash one.  open, close, push_dev, push and destroy are the entries above.  A stream keeps 64 counters, the total
 * weight, the one unfinished token and the held-back byte on the device (ucfp_text_streams_state_bytes_sim, about 2 KiB).
 * CONTRACT.  Let B be the concatenation of a stream's chunks, however they are cut.  The final record and status equal
 * those of ucfp_text_simhash_batch(mode) -- with a table, of ucfp_text_simhash_idf_batch(table, mode, UCFP_TEXT_TOK_WORD)
 * -- on the one document B, byte for byte, whenever every token of B has at most UCFP_TEXT_MAX_WINDOW_BYTES canonical
 * bytes; above that limit, what the MinHash streams promise (the window is the single token, text.rs:277-280: SimHash
 * hashes tokens, not shingles).  The held-back byte, d_status, the sticky statuses (UCFP_TEXT_NEEDS_HOST, which wins, and
 * UCFP_E_UNSUPPORTED), UCFP_E_MODALITY on a final entry only, locking, ordering and everything said of UTF-8 STREAMS are
 * those of the MinHash streams.  With a table UCFP_E_MODALITY also ends a stream whose tokens weigh 0 in all (T9.3).
 *   - BYTE LIMIT.  A SimHash stream carries fewer than UCFP_TEXT_SIMHASH_STREAM_LIMIT_BYTES bytes: the record compares
 *     2 x a 32-bit count, and the weighted sums hold 2^31 weights.  n bytes make at most 4 n canonical bytes
 *     (ucfp_text_canon_bound) and a token costs two of them, its separator included, so fewer than 2^30 bytes keep the
 *     token count below 2^31.  A push that would reach the limit fails with UCFP_E_INVALID and changes no state.
 *   - TABLE.  The set reads the table at every push and does not own it: the table must outlive the set.  A push while
 *     the table is not final (T9.6) fails with UCFP_E_INVALID and changes no state.  Changing a table's weights in the
 *     middle of a stream gives a record that no offline call gives: tokens are weighed when their push runs. */
#define UCFP_TEXT_SIMHASH_STREAM_LIMIT_BYTES 0x40000000ull
/* text.rs:328-421 behind text.rs:645-730.  flags: 0 or UCFP_TEXT_STREAMS_UTF8, then max_push_bytes in [1, 2^28], as
 * ucfp_text_streams_create_ex; unknown flags -> UCFP_E_INVALID.  table == NULL: TF records (text.rs:328-343); a table on
 * the context's device: the weighted records of T9 (text.rs:344-362).  max_streams in [1, 2^20].  Fails with
 * UCFP_E_INDEX without a gfx950 device (no CPU fallback). */
int ucfp_text_streams_create_sim(ucfp_ctx* ctx, uint32_t max_streams, uint32_t flags, uint64_t max_push_bytes,
                                 const ucfp_idf_table* table, ucfp_text_streams** out);
/* text.rs:277-280, :645-730.  Host-only: bytes of a final record of this set, UCFP_MINHASH_BYTES or UCFP_SIMHASH_BYTES
 * (0 for NULL).  ucfp_text_streams_push_dev writes d_out with this stride (n x this many bytes) and
 * ucfp_text_streams_push copies this many bytes to `out`. */
size_t ucfp_text_streams_record_bytes(const ucfp_text_streams* s);
/* text.rs:328-421, :645-730.  Host-only: device bytes a SimHash set holds per stream; weighted != 0: a set with a table
 * (64-bit sums). */
size_t ucfp_text_streams_state_bytes_sim(uint32_t flags, int weighted);

/* ---- the first half of UCFP_TEXT_RAW_UTF8 on its own: documents -> canonical token strings ----
 * What the Rust host otherwise does with txtfp's canonicaliser and tokeniser before text::fingerprint_minhash_with
 * (src/modality/text.rs:112-114,182-236).  tok_offsets has n + 1 entries (tok_offsets[0] = 0); document i's tokens, joined
 * by single spaces, are tokens[tok_offsets[i] .. tok_offsets[i + 1]); status[i] is 0 or UCFP_TEXT_NEEDS_HOST (then the
 * document has no token bytes).  The blob never exceeds ucfp_text_canon_bound(bytes of the batch) = 4 x the input. */
/* src/modality/text.rs:112-114,182-236; host code, no device */
size_t ucfp_text_canon_bound(size_t n_bytes);
/* src/modality/text.rs:112-114,182-236; d_tokens holds ucfp_text_canon_bound(d_offsets[n] - d_offsets[0]) bytes; no
 * workspace, no synchronisation: three launches on `stream` */
int ucfp_text_canon_batch_dev(ucfp_ctx* ctx, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, uint8_t* d_tokens,
                              uint64_t* d_tok_offsets, int32_t* d_status, void* stream);
/* src/modality/text.rs:112-114,182-236; host pointers; UCFP_E_INVALID when the blob is larger than tokens_cap */
int ucfp_text_canon_batch(ucfp_ctx* ctx, const uint8_t* utf8, const uint64_t* offsets, size_t n, uint8_t* tokens,
                          size_t tokens_cap, uint64_t* tok_offsets, int32_t* status);
/* Host code, no device: the compiled code-point table (include/ucfp_text_utab.h).  Returns 1 when cp is covered (U1), else
 * 0.  Covered: out_cps[0 .. *n) = M(cp), 0 .. 6 code points; when *n == 1, *cls_flags describes that one canonical code
 * point -- bits 0-3 Word_Break class (0 Other, 1 ALetter, 2 Hebrew_Letter, 3 Numeric, 4 Katakana, 5 ExtendNumLet,
 * 6 MidLetter, 7 MidNum, 8 MidNumLet, 9 Single_Quote, 10 Double_Quote), bit 4 str.isalnum, bit 5 vowel of the apostrophe
 * tailoring -- otherwise 0: every code point of M(cp) is covered and maps to itself, look it up in turn.
 * ucfp_text_utab_versions: "unicodedata <version> regex <version>" the table was generated with. */
int ucfp_text_utab_lookup(uint32_t cp, uint32_t out_cps[8], uint32_t* n, uint32_t* cls_flags);
const char* ucfp_text_utab_versions(void);

/* ---- HTML pages -> text: the `preprocess = html` stage of the text route on its own (rules M1-M8) ----
 * What the Rust host otherwise does with txtfp::html_to_text before it fingerprints a page (TextOpts.preprocess,
 * src/modality/text.rs:85-96,751-767, behind POST /v1/ingest/text/{tid}/{rid}/preprocess/html,
 * src/server/handlers.rs:628-699).  txtfp is not available, so the rules are this library's own (parity unpinned): tags,
 * comments, declarations and script / style bodies are dropped, a tag outside the inline set leaves a space, the 252
 * named references of HTML 4, `apos` and the numeric ones are decoded, runs of white space become one space.  A total
 * function from bytes to bytes: no status, no hand-back; bytes >= 0x80 pass through (UTF-8 is validated by whatever
 * consumes the text).  Same blob + n + 1 byte offsets shape as the MinHash calls; text_offsets has n + 1 entries
 * (text_offsets[0] = 0) and document i's text is text[text_offsets[i] .. text_offsets[i + 1]), so the output feeds
 * ucfp_text_minhash_batch_dev and its kin as it is.  flags[i] (may be NULL): bit 0 (UCFP_TEXT_HTML_NON_ASCII) the text holds
 * a byte >= 0x80; bit 1 (UCFP_TEXT_HTML_OPEN_MARKUP) the document ended inside markup, which was dropped to the end.  The
 * text is never longer than the page. */
#define UCFP_TEXT_HTML_NON_ASCII 1u
#define UCFP_TEXT_HTML_OPEN_MARKUP 2u
/* src/modality/text.rs:751-767, src/server/handlers.rs:628-699; host code, no device: returns n_bytes */
size_t ucfp_text_html_bound(size_t n_bytes);
/* src/modality/text.rs:751-767, src/server/handlers.rs:628-699; device pointers; d_text holds
 * ucfp_text_html_bound(d_offsets[n] - d_offsets[0]) bytes; no workspace, no synchronisation: three launches on `stream`;
 * n = 0 launches one and writes d_text_offsets[0] = 0 */
int ucfp_text_html_batch_dev(ucfp_ctx* ctx, const uint8_t* d_html, const uint64_t* d_offsets, size_t n, uint8_t* d_text,
                             uint64_t* d_text_offsets, uint32_t* d_flags, void* stream);
/* src/modality/text.rs:751-767, src/server/handlers.rs:628-699; host pointers; UCFP_E_INVALID when the text is larger
 * than text_cap */
int ucfp_text_html_batch(ucfp_ctx* ctx, const uint8_t* html, const uint64_t* offsets, size_t n, uint8_t* text, size_t text_cap,
                         uint64_t* text_offsets, uint32_t* flags);
/* src/modality/text.rs:751-767, src/server/handlers.rs:628-699; host code, no device: the compiled table of named
 * references (include/ucfp_text_html_tab.h).  Returns 1 and *cp when name[0 .. len) is one of them (case-sensitive), else 0. */
int ucfp_text_html_entity(const char* name, size_t len, uint32_t* cp);

/* ---- TLSH 128/1 (the `tlsh` arm of the text route, src/modality/text.rs:452-484, tag "tlsh-128-1") ----
 * The digest of a BYTE STRING: for a text record the UTF-8 of the canonicalised, preprocessed text (the reference's
 * tokenizer tag "tlsh-bytes"); there is no `mode`, bytes are bytes, 0x00 and 0xff included.  Same blob + n + 1 byte
 * offsets shape as the MinHash calls.  A record is UCFP_TLSH_BYTES bytes in the order of the published hex string:
 * swap(checksum), swap(L), (Q1 << 4) | Q2, code[31] .. code[0] (swap exchanges the nibbles); the reference stores
 * "T1" + the 70 upper-case hex digits of these bytes.
 * status[i] (may be NULL): 0, or UCFP_E_MODALITY for a document that TLSH refuses -- shorter than 50 bytes, at most 64
 * of the 128 buckets non-zero, or 2^31 bytes and longer; its record is all zero.  n = 0 is a no-op.  One wave hashes
 * one document whatever its length.
 * PARITY: bit-exact against the restatement of the published algorithm in tests/tlsh_ref.py only; no digest made by
 * another implementation was available. */
#define UCFP_TLSH_BYTES 35u
#define UCFP_TLSH_MAX_DISTANCE 2473u /* 1536 (L) + 84 + 84 (Q1, Q2) + 1 (checksum) + 768 (body) */
/* src/modality/text.rs:452-484 */
int ucfp_text_tlsh_batch_dev(ucfp_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets, size_t n, uint8_t* d_out,
                             int32_t* d_status, void* stream);
/* src/modality/text.rs:452-484; host pointers */
int ucfp_text_tlsh_batch(ucfp_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, size_t n, uint8_t* out,
                         int32_t* status);
/* Host-only (no device needed).  The L byte of a document of n bytes, from the committed table of class boundaries
 * (include/ucfp_tlsh_ltab.h); the TLSH distance of two 35-byte digests, 0 .. UCFP_TLSH_MAX_DISTANCE (a NULL argument
 * gives UCFP_TLSH_MAX_DISTANCE). */
uint32_t ucfp_tlsh_lvalue(uint64_t n);
uint32_t ucfp_tlsh_distance(const uint8_t* a, const uint8_t* b);

/* TLSH-distance search: the k <= UCFP_INDEX_MAX_K rows of a tenant nearest to each query digest, EXACT, ties included.
 *   rows / queries   packed 35-byte digests; any 35 bytes are a valid row
 *   upsert           a known id replaces its row; tenants are isolated; delete reports how many ids it removed
 *   query            rows with distance > max_distance are left out (UINT32_MAX: no cut); order (distance ascending,
 *                    id ascending); score = (float)(2473 - distance) / 2473.0f.  out_ids / out_dist / out_scores: nq x k,
 *                    unused slots UCFP_INVALID_ID / UINT32_MAX / -1; out_n: nq.  An unknown tenant, k = 0 or nq = 0
 *                    gives 0 hits.
 * Mutations are host bookkeeping; the device rows of a tenant are rebuilt at its next query (or by flush).  The
 * *_dev calls take device pointers and a stream and are stream-ordered.  Not built: sharding over GPUs, a search
 * micro-batcher, save / load. */
typedef struct ucfp_tlsh_index ucfp_tlsh_index;
int ucfp_tlsh_index_create(ucfp_ctx* ctx, uint32_t flags, ucfp_tlsh_index** out);
void ucfp_tlsh_index_destroy(ucfp_tlsh_index* ix);
int ucfp_tlsh_index_upsert(ucfp_tlsh_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* digests, size_t n);
int ucfp_tlsh_index_upsert_dev(ucfp_tlsh_index* ix, uint32_t tenant, const uint64_t* d_ids, const uint8_t* d_digests,
                               size_t n, void* stream);
int ucfp_tlsh_index_delete(ucfp_tlsh_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed);
int ucfp_tlsh_index_size(ucfp_tlsh_index* ix, uint32_t tenant, size_t* rows);
int ucfp_tlsh_index_flush(ucfp_tlsh_index* ix);
int ucfp_tlsh_index_query(ucfp_tlsh_index* ix, uint32_t tenant, const uint8_t* digests, size_t nq, uint32_t k,
                          uint32_t max_distance, uint64_t* out_ids, uint32_t* out_dist, float* out_scores, uint32_t* out_n);
int ucfp_tlsh_index_query_dev(ucfp_tlsh_index* ix, uint32_t tenant, const uint8_t* d_digests, size_t nq, uint32_t k,
                              uint32_t max_distance, uint64_t* d_out_ids, uint32_t* d_out_dist, float* d_out_scores,
                              uint32_t* d_out_n, void* stream);

/* ---- MinHash search: the k <= UCFP_INDEX_MAX_K MinHash-128 records of a tenant that agree with each query
 * record in the most slots, EXACT, ties included.  The reference produces these records (`minhash-h128`,
 * src/modality/text.rs:172; re-tagged `minhash-lsh-h128`, :428-446) and has no search over them; ucfp_lsh_* above is the
 * approximate, build-once counterpart.
 *   rows / queries   UCFP_MINHASH_BYTES records; the 8 header bytes are neither compared nor validated
 *   agree(q, r)      the number of i < 128 with slot_i(q) == slot_i(r): all 64 bits, the same index only (the score
 *                    numerator of ucfp_lsh_query_dev, the `agree` of ucfp_lsh_dedup_dev)
 *   upsert           a known id replaces its row; tenants are isolated; delete reports how many ids it removed
 *   query            rows with agree < min_agree are left out (0: every row is a hit; above 128: UCFP_E_INVALID); order
 *                    (agree descending, id ascending); score = (float)agree / 128.0f.  out_ids / out_agree / out_scores:
 *                    nq x k, unused slots UCFP_INVALID_ID / UINT32_MAX / -1; out_n: nq.  An unknown tenant, an empty
 *                    tenant, k = 0 or nq = 0 gives 0 hits.
 * Mutations are host bookkeeping; the device rows of a tenant are rebuilt at its next query (or by flush).  The
 * *_dev calls take device pointers and a stream and are stream-ordered (no synchronisation beyond workspace growth and
 * the rebuild after a mutation).  The key matrix of one pass is capped at 1 GiB; UCFP_MINHASH_KEY_BYTES in the
 * environment, read once at creation, overrides the cap (floor 4096).  Not built: a compact filter plane, device-resident
 * appends, sharding over GPUs, a search micro-batcher, save / load. */
typedef struct ucfp_minhash_index ucfp_minhash_index;
/* DESIGN.md A17; flags must be 0 */
int ucfp_minhash_index_create(ucfp_ctx* ctx, uint32_t flags, ucfp_minhash_index** out);
/* DESIGN.md A17 */
void ucfp_minhash_index_destroy(ucfp_minhash_index* ix);
/* DESIGN.md A17 */
int ucfp_minhash_index_upsert(ucfp_minhash_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* records, size_t n);
/* DESIGN.md A17 */
int ucfp_minhash_index_upsert_dev(ucfp_minhash_index* ix, uint32_t tenant, const uint64_t* d_ids, const uint8_t* d_records,
                                  size_t n, void* stream);
/* DESIGN.md A17 */
int ucfp_minhash_index_delete(ucfp_minhash_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed);
/* DESIGN.md A17 */
int ucfp_minhash_index_size(ucfp_minhash_index* ix, uint32_t tenant, size_t* rows);
/* DESIGN.md A17 */
int ucfp_minhash_index_flush(ucfp_minhash_index* ix);
/* DESIGN.md A17; host pointers */
int ucfp_minhash_index_query(ucfp_minhash_index* ix, uint32_t tenant, const uint8_t* records, size_t nq, uint32_t k,
                             uint32_t min_agree, uint64_t* out_ids, uint32_t* out_agree, float* out_scores, uint32_t* out_n);
/* DESIGN.md A17; device pointers, stream-ordered */
int ucfp_minhash_index_query_dev(ucfp_minhash_index* ix, uint32_t tenant, const uint8_t* d_records, size_t nq, uint32_t k,
                                 uint32_t min_agree, uint64_t* d_out_ids, uint32_t* d_out_agree, float* d_out_scores,
                                 uint32_t* d_out_n, void* stream);
/* DESIGN.md A17; host-only (no device needed): agree of two records, 0 .. 128 (a NULL argument gives 0) */
uint32_t ucfp_minhash_agree(const uint8_t* a, const uint8_t* b);
/* Records of h slots (the records of text.rs:182-236 at any H).  An index holds records of ONE h, fixed
 * at creation: rows and queries are UCFP_MINHASH_RECORD_BYTES(h) bytes, agree counts the i < h, min_agree above h is
 * UCFP_E_INVALID and score = (float)agree / (float)h (one f32 division; at h = 128 the agree / 128.0f above, bit for bit).
 * ucfp_minhash_index_create is create_h with h = 128; every other ucfp_minhash_index_* call takes either handle. */
int ucfp_minhash_index_create_h(ucfp_ctx* ctx, uint32_t flags, uint32_t h, ucfp_minhash_index** out);
/* the h of a handle (0 for NULL) */
uint32_t ucfp_minhash_index_slots(ucfp_minhash_index* ix);
/* host-only: agree of two records of h slots, 0 .. h (a NULL argument or an invalid h gives 0); text.rs:182-236 */
uint32_t ucfp_minhash_agree_h(const uint8_t* a, const uint8_t* b, uint32_t h);

/* ---- image search over whole records: global and block hashes scored together ----
 * The reference threads a compare-time MultiHashConfig through its adapter and its DTO (src/modality/image.rs:90-104,
 * src/server/dto.rs:462-480: phash_weight, dhash_weight, ahash_weight, global_weight, block_weight,
 * block_distance_threshold) and has no matcher that reads it; this is that matcher.  Rows and queries are the records
 * ucfp_image_hash_batch* writes: 168 bytes (17 u64 LE codes: the global hash at byte 32, the 16 block hashes behind it)
 * or the 536-byte bundle (3 x 17 codes, records at bytes 32, 200, 368 in the order ahash, phash, dhash); `exact` takes no
 * part.  Per algorithm, with g and d_b the Hamming distances of the global and of block b and T the threshold:
 *   S = sum over b of (d_b <= T ? 64 - d_b : 0);  sg = (float)(64 - g) * 2^-6;  sb = (float)S * 2^-10
 *   s = (global_weight * sg) + (block_weight * sb)
 * score = s for a 168-byte index (the three algorithm weights are then ignored), and for a bundle index
 *   ((ahash_weight * s_ahash) + (phash_weight * s_phash)) + (dhash_weight * s_dhash)
 * every product and sum rounded to f32 on its own; no normalisation, no clamp.  The defaults (ours; the reference
 * states none) are 0.1 / 0.6 / 0.3, 0.4 / 0.6, T = 32, min_score = 0: a record against itself then scores 1.0f.
 * UCFP_E_INVALID: a weight that is not finite or outside [0, 1] (-0 counts as 0), all three algorithm weights zero on a
 * bundle, global_weight and block_weight both zero, block_distance_threshold > 64, min_score not finite or negative.
 * PARITY: unpinned -- imgfprint's own compare is not in the tree; bit-exact against the restatement in
 * tests/image_match_ref.py only. */
typedef struct ucfp_image_match_config {
    float ahash_weight;
    float phash_weight;
    float dhash_weight;
    float global_weight;
    float block_weight;
    uint32_t block_distance_threshold;
    float min_score; /* hits need score >= min_score */
} ucfp_image_match_config;
/* Host-only (no device needed): the defaults; the score of one pair of records of `algo` (one of UCFP_IMG_*; cfg NULL =
 * defaults, validated as above). */
void ucfp_image_match_config_default(ucfp_image_match_config* cfg);
int ucfp_image_match_score(const uint8_t* a, const uint8_t* b, uint32_t algo, const ucfp_image_match_config* cfg, float* out);

/* The index: the k <= UCFP_INDEX_MAX_K rows of a tenant that score highest against each query record, EXACT, ties included.
 *   create           algo: one of UCFP_IMG_{AHASH,PHASH,DHASH,MULTI}, which fixes the record size (168 or 536 bytes);
 *                    flags must be 0
 *   upsert           a known id replaces its row; tenants are isolated; delete reports how many ids it removed;
 *                    upsert_dev takes the records ucfp_image_hash_batch_dev wrote
 *   query            cfg is a per-query setting (NULL = defaults), not index state.  Rows with score < min_score are left
 *                    out; order (score descending, id ascending).  out_ids / out_scores: nq x k, unused slots
 *                    UCFP_INVALID_ID / -1; out_n: nq.  An unknown tenant, k = 0 or nq = 0 gives 0 hits.
 * Mutations are host bookkeeping; the device rows of a tenant are rebuilt at its next query (or by flush).  The
 * *_dev calls take device pointers and a stream and are stream-ordered.  A tenant holds fewer than 2^31 rows; the row
 * table lives on the host; one GPU.  Not built: sharding over GPUs, a search micro-batcher, save / load. */
typedef struct ucfp_image_match_index ucfp_image_match_index;
int ucfp_image_match_index_create(ucfp_ctx* ctx, uint32_t algo, uint32_t flags, ucfp_image_match_index** out);
void ucfp_image_match_index_destroy(ucfp_image_match_index* ix);
int ucfp_image_match_index_upsert(ucfp_image_match_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* records,
                                  size_t n);
int ucfp_image_match_index_upsert_dev(ucfp_image_match_index* ix, uint32_t tenant, const uint64_t* d_ids,
                                      const uint8_t* d_records, size_t n, void* stream);
int ucfp_image_match_index_delete(ucfp_image_match_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed);
int ucfp_image_match_index_size(ucfp_image_match_index* ix, uint32_t tenant, size_t* rows);
int ucfp_image_match_index_flush(ucfp_image_match_index* ix);
int ucfp_image_match_index_query(ucfp_image_match_index* ix, uint32_t tenant, const uint8_t* records, size_t nq, uint32_t k,
                                 const ucfp_image_match_config* cfg, uint64_t* out_ids, float* out_scores, uint32_t* out_n);
int ucfp_image_match_index_query_dev(ucfp_image_match_index* ix, uint32_t tenant, const uint8_t* d_records, size_t nq, uint32_t k,
                                     const ucfp_image_match_config* cfg, uint64_t* d_out_ids, float* d_out_scores,
                                     uint32_t* d_out_n, void* stream);

/* Host micro-batcher for documents: the caller side of handlers::ingest_text
 * (src/server/handlers.rs:304-460) fingerprints one document per request thread, up to 512 in flight
 * (src/bin/ucfp.rs:267).  submit() is BLOCKING and thread-safe: concurrent calls are packed back to back into one
 * pinned blob + offset table, one H2D copy, one ucfp_text_*_batch_dev launch and one D2H copy -- at most max_batch
 * documents or max_bytes of text per flush, flushed no later than max_delay_us after the first pending document.
 * One (algorithm, mode, k) per batcher: the host keeps one for RAW_ASCII and one for PRETOKENIZED documents.
 * `out` receives UCFP_MINHASH_BYTES or UCFP_SIMHASH_BYTES; *status as in the batch calls. */
#define UCFP_TEXT_ALGO_MINHASH 1
#define UCFP_TEXT_ALGO_SIMHASH 2
typedef struct ucfp_text_batcher ucfp_text_batcher;
int ucfp_text_batcher_create(ucfp_ctx* ctx, uint32_t algo, int mode, uint32_t shingle_k, size_t max_batch, size_t max_bytes,
                             uint32_t max_delay_us, ucfp_text_batcher** out);
void ucfp_text_batcher_destroy(ucfp_text_batcher* b);
int ucfp_text_batcher_submit(ucfp_text_batcher* b, const uint8_t* utf8, size_t len, uint8_t* out, int32_t* status);
int ucfp_text_batcher_stats(ucfp_text_batcher* b, uint64_t* batches, uint64_t* items);

/* ---- banded MinHash LSH (the reference only re-tags the record, text.rs:437-446) ----
 * key_b = FNV-style fold of slots [b*rows, (b+1)*rows) + splitmix64 finaliser; bands*rows <= 128.
 * ucfp_text_lsh_band_keys_dev writes keys band-major: d_keys[b*n + doc]. */
int ucfp_text_lsh_band_keys_dev(ucfp_ctx* ctx, const uint8_t* d_records, size_t n, uint32_t bands, uint32_t rows,
                                uint64_t* d_keys, void* stream);
typedef struct ucfp_lsh ucfp_lsh;
/* cand_per_band: rows examined per band per query (0 = 64). */
int ucfp_lsh_create(ucfp_ctx* ctx, uint32_t bands, uint32_t rows, uint32_t cand_per_band, ucfp_lsh** out);
void ucfp_lsh_destroy(ucfp_lsh* lsh);
/* (Re)build from n device-resident 1032-byte MinHash records and their record ids. */
int ucfp_lsh_build_dev(ucfp_lsh* lsh, const uint64_t* d_ids, const uint8_t* d_records, size_t n, void* stream);
/* For each query record: candidates = rows sharing a band key (first cand_per_band per band, at most
 * 1024 in total); score = equal slots / 128; best k by (score desc, id asc). */
int ucfp_lsh_query_dev(ucfp_lsh* lsh, const uint8_t* d_query_records, size_t nq, uint32_t k, uint64_t* d_out_ids,
                       float* d_out_scores, uint32_t* d_out_counts, void* stream);
/* Near-duplicate clusters of the rows 0 .. n-1 of the last ucfp_lsh_build_dev, all on the device.
 * agree(a, c) = number of i < 128 with slot_i(a) == slot_i(c) (all 128 slots, also those no band covers).
 *   candidates  per band, per maximal run of equal keys in the sorted table (rows r_0 < r_1 < ... < r_{m-1}, the sort
 *               is stable): the pairs (r_i, r_j) with 0 < j - i <= span.  span = 0 means 16, span = UINT32_MAX every
 *               pair of the run.  Runs are runs of equal KEYS, so a 64-bit key collision makes a run as well.
 *   edges       candidates with agree >= min_agree, 1 <= min_agree <= 128
 *   clusters    connected components of the edge graph: labels[row] = smallest row of the component,
 *               keep[row] = (labels[row] == row), rep_ids[row] = ids[labels[row]]
 *   stats       [0] pairs = candidates summed over bands (a pair counts once per band it appears in),
 *               [1] clusters = rows with keep, [2] duplicates = n - clusters, [3] largest = size of the largest cluster
 * Every output is a function of the build's input alone.  Stream-ordered; the only synchronisation is what growing the
 * workspace needs.  The workspace lives in the object: one dedup in flight per ucfp_lsh.  An index never built or built
 * empty: UCFP_OK, stats all zero. */
int ucfp_lsh_dedup_dev(ucfp_lsh* lsh, uint32_t min_agree, uint32_t span,
                       uint32_t* d_out_labels,   /* n, required            */
                       uint64_t* d_out_rep_ids,  /* n, may be NULL         */
                       uint8_t*  d_out_keep,     /* n, may be NULL         */
                       uint64_t* d_out_stats,    /* 4, may be NULL         */
                       void* stream);

/* ---- landmark index over Wang hashes (the reference has no audio matcher) ----
 * Records and queries are sets of landmarks: 8 bytes each, u32 LE hash then u32 LE t (UCFP_WANG_HASH_BYTES), t < 2^31.
 * Item i of a batch is landmarks[offsets[i] .. offsets[i+1]) with BYTE offsets: offsets[0] = 0, non-decreasing,
 * multiples of 8; n + 1 entries.  Duplicate (hash, t) pairs count once.  Within a tenant, P(h) = distinct (record, t)
 * postings of hash h; an index with max_postings > 0 ignores every h with P(h) > max_postings (0 = no cap).
 * votes(r) = max over d of |{(h, t) in Q : (h, t + d) in R_r}|, offset(r) = the smallest d attaining it (the position of
 * the query's frame 0 in the record, in frames).  Hits: votes >= max(min_votes, 1), ordered (votes desc, id asc), first
 * k <= UCFP_INDEX_MAX_K; score = (float)votes / (float)|Q|.  Unused output slots: id UINT64_MAX, votes 0, offset 0,
 * score -1.  An empty query, k = 0 or an unknown tenant gives 0 hits; bad offsets or t >= 2^31 give UCFP_E_INVALID.
 * Upsert of a known id replaces its set, delete removes it; postings are rebuilt lazily at the next query, size or
 * flush of a changed tenant.  Queries read the checked sizes and the vote count of each query back to the host (two
 * synchronisations of `stream`) to size their buffers; the rest of a query is asynchronous.  upsert_dev copies its
 * inputs to the host record table (it synchronises `stream`).  flags: 0. */
typedef struct ucfp_landmark_index ucfp_landmark_index;
int ucfp_landmark_index_create(ucfp_ctx* ctx, uint32_t max_postings, uint32_t flags, ucfp_landmark_index** out);
void ucfp_landmark_index_destroy(ucfp_landmark_index* ix);
int ucfp_landmark_index_upsert(ucfp_landmark_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* landmarks,
                               const uint64_t* offsets, size_t n);
int ucfp_landmark_index_upsert_dev(ucfp_landmark_index* ix, uint32_t tenant, const uint64_t* d_ids,
                                   const uint8_t* d_landmarks, const uint64_t* d_offsets, size_t n, void* stream);
int ucfp_landmark_index_delete(ucfp_landmark_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed);
/* records = live records (empty ones included); postings = sum of P(h) (rebuilds a changed tenant). */
int ucfp_landmark_index_size(ucfp_landmark_index* ix, uint32_t tenant, size_t* records, size_t* postings);
int ucfp_landmark_index_flush(ucfp_landmark_index* ix);
/* nq ragged queries; out_ids / out_votes / out_offsets / out_scores are nq x k; out_n[q] = hits of query q. */
int ucfp_landmark_index_query(ucfp_landmark_index* ix, uint32_t tenant, const uint8_t* landmarks, const uint64_t* offsets,
                              size_t nq, uint32_t k, uint32_t min_votes, uint64_t* out_ids, uint32_t* out_votes,
                              int32_t* out_offsets, float* out_scores, uint32_t* out_n);
int ucfp_landmark_index_query_dev(ucfp_landmark_index* ix, uint32_t tenant, const uint8_t* d_landmarks,
                                  const uint64_t* d_offsets, size_t nq, uint32_t k, uint32_t min_votes, uint64_t* d_out_ids,
                                  uint32_t* d_out_votes, int32_t* d_out_offsets, float* d_out_scores, uint32_t* d_out_n,
                                  void* stream);

/* ---- Panako triplet index with a (scale, offset) vote (the reference has no audio matcher) ----
 * Identification that survives a change of tempo.  Records and queries are sequences of Panako records: 16 bytes each,
 * u32 LE hash, t_a, t_b, t_c (UCFP_PANAKO_HASH_BYTES).  Item i of a batch is records[offsets[i] .. offsets[i+1]) with BYTE
 * offsets: offsets[0] = 0, non-decreasing, multiples of 16; n + 1 entries.  The set of an item is its distinct triples
 * (h, a, d) with a = t_a and d = t_c - t_a; t_b is not used (r = h & 31 stands for it).  UCFP_E_INVALID before anything
 * runs: bad offsets, d outside 1 ... 1023, t_a >= 2^31 in a record, t_a >= 2^28 in a query (every offset then fits an
 * int32), a match config out of range.  |Q| = the distinct triples of a query.  All arithmetic below is in signed
 * 64-bit integers; scales are in units of 1/256.
 *   hypotheses  s = scale_min + j * scale_step <= scale_max, 64 <= scale_min <= scale_max <= 1024, scale_step >= 1, at
 *               most 64 of them; window W in 1 ... 256; slack in 0 ... 8; r_slack 0 or 1.  config NULL = 204, 320, 4,
 *               16, 2, 1.
 *   probes      a query triple with hash h probes (h & ~31) | r' for r' = max(0, r - r_slack) ... min(31, r + r_slack).
 *               Within a tenant P(h') = distinct (record, a', d') postings of h' over the live records; an index with
 *               max_postings > 0 ignores every probed h' with P(h') > max_postings (0 = no cap).
 *   votes       a match is a pair (query triple (h, a, d), posting (r, h', a', d')) with h' probed and not ignored.  It
 *               supports s iff |256 d' - s d| <= 256 slack; its offset under s is a' - ((s a + 128) >> 8).
 *               count(r, s, o) = matches of record r that support s with o <= offset < o + W; PAIRS are counted: a
 *               query triple that meets several postings counts once for each.  votes(r) = the maximum over the
 *               hypotheses s and over every o that is the offset of some supporting match; (scale(r), offset(r)) = the
 *               maximiser with the smallest (|s - 256|, s, o), compared in that order.
 *   hits        votes >= max(min_votes, 1), ordered (votes desc, id asc), first k <= UCFP_INDEX_MAX_K;
 *               score = (float)votes / (float)|Q|, which may exceed 1 because pairs are counted.  Unused output slots:
 *               id UINT64_MAX, votes 0, offset 0, scale 0, score -1.  An empty query, k = 0 or an unknown tenant gives
 *               0 hits.
 * Upsert of a known id replaces its set, delete removes it, an empty record is stored and counted; postings are rebuilt
 * lazily at the next query, size or flush of a changed tenant.  Limits: at most 2^23 records per tenant (the ordinal
 * bits of a posting; UCFP_E_INVALID at the rebuild), a tenant below 2^32 - 1 triples.  UCFP_E_UNSUPPORTED: a query whose
 * expanded votes (matches x supported hypotheses) reach 2^32, a batch whose queries above
 * ucfp_panako_index_lds_votes() expand to 2^32 - 1 votes or more in all, a single window that holds 2^26 votes or more.
 * A query with at most ucfp_panako_index_lds_votes() expanded votes is answered in on-chip memory, a larger one through
 * global memory; the answers do not depend on the path.  Queries read the checked sizes, the input flags and the vote
 * count of each query back to the host (three synchronisations of `stream`); upsert_dev copies its inputs to the host
 * record table (it synchronises `stream`).  flags: 0. */
typedef struct ucfp_panako_match_config {
    uint32_t scale_min, scale_max; /* 64 <= min <= max <= 1024, units of 1/256 */
    uint32_t scale_step;           /* >= 1; (max - min) / step + 1 <= 64 */
    uint32_t window;               /* 1 ... 256 frames */
    uint32_t slack;                /* 0 ... 8 frames on d' */
    uint32_t r_slack;              /* 0 or 1 on the ratio bits of the hash */
} ucfp_panako_match_config;
typedef struct ucfp_panako_index ucfp_panako_index;
/* expanded votes up to which a query stays in on-chip memory.  Host only. */
uint32_t ucfp_panako_index_lds_votes(void);
int ucfp_panako_index_create(ucfp_ctx* ctx, uint32_t max_postings, uint32_t flags, ucfp_panako_index** out);
void ucfp_panako_index_destroy(ucfp_panako_index* ix);
int ucfp_panako_index_upsert(ucfp_panako_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* records,
                             const uint64_t* offsets, size_t n);
int ucfp_panako_index_upsert_dev(ucfp_panako_index* ix, uint32_t tenant, const uint64_t* d_ids, const uint8_t* d_records,
                                 const uint64_t* d_offsets, size_t n, void* stream);
int ucfp_panako_index_delete(ucfp_panako_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed);
/* records = live records (empty ones included); postings = sum of P(h) (rebuilds a changed tenant). */
int ucfp_panako_index_size(ucfp_panako_index* ix, uint32_t tenant, size_t* records, size_t* postings);
int ucfp_panako_index_flush(ucfp_panako_index* ix);
/* nq ragged queries; out_ids / out_votes / out_offsets / out_scales / out_scores are nq x k; out_n[q] = hits of query q. */
int ucfp_panako_index_query(ucfp_panako_index* ix, uint32_t tenant, const uint8_t* records, const uint64_t* offsets, size_t nq,
                            uint32_t k, uint32_t min_votes, const ucfp_panako_match_config* cfg, uint64_t* out_ids,
                            uint32_t* out_votes, int32_t* out_offsets, uint32_t* out_scales, float* out_scores,
                            uint32_t* out_n);
int ucfp_panako_index_query_dev(ucfp_panako_index* ix, uint32_t tenant, const uint8_t* d_records, const uint64_t* d_offsets,
                                size_t nq, uint32_t k, uint32_t min_votes, const ucfp_panako_match_config* cfg,
                                uint64_t* d_out_ids, uint32_t* d_out_votes, int32_t* d_out_offsets, uint32_t* d_out_scales,
                                float* d_out_scores, uint32_t* d_out_n, void* stream);

/* ---- The same vote for RESAMPLED copies: the bins follow the scale ----
 * A copy played at another speed through a resampler (a tape off speed, a sped-up upload) has its times divided by the
 * speed and every frequency multiplied by it, so the three 9-bit bins of its hashes (h = k_a << 23 | k_b << 14 |
 * k_c << 5 | r) move and the probes above meet nothing.  Two more match parameters: bins (0 = kept, the vote above;
 * 1 = scaled) and f_slack in 0 ... 3, which must be 0 when bins = 0.  Everything of A14 that is not named here is
 * unchanged; all arithmetic is in signed integers.
 *   bin map     of hypothesis s (record frames per query frame = the speed the query was played at, in 1/256):
 *               B_s(k) = (512 k + s) / (2 s) in integer division = round(256 k / s); non-increasing in s; B_256(k) = k.
 *   votes       with bins = 1 a match is a pair (query triple (h, a, d) with bins k_a, k_b, k_c and ratio r, posting
 *               (record, h', a', d') with bins k_a', k_b', k_c' and ratio r') whose h' is not ignored (P(h') <=
 *               max_postings, as above).  It supports s iff |k_x' - B_s(k_x)| <= f_slack for x = a, b, c and
 *               |r' - r| <= r_slack and |256 d' - s d| <= 256 slack; its offset under s is a' - ((s a + 128) >> 8).
 *               Every (match, supported s) is one vote; count, votes, (scale, offset), hits, score, |Q| and the limits
 *               on expanded votes are those above, word for word.
 *   intervals   for 64 <= s <= 1024, |k' - B_s(k)| <= f holds iff 512 k / (2 k' + 2 f + 1) + 1 <= s and, when
 *               k' - f >= 1, s <= 512 k / (2 (k' - f) - 1): the hypotheses of a match are one interval, as above.
 * With bins = 1, f_slack = 0 and the single hypothesis 256 the answers are those of bins = 0.  config NULL = 204, 320,
 * 4, 16, 2, 1 with bins = 0.  UCFP_E_INVALID before anything runs: bins > 1, f_slack > 3, f_slack != 0 with bins = 0.
 * ucfp_panako_index_query and _query_dev forward here with bins = 0; their struct keeps its layout.  Independent
 * changes of pitch and tempo are not covered: a caller who does not know which change a copy went through asks with
 * bins = 0 and with bins = 1. */
typedef struct ucfp_panako_match_config_ex {
    uint32_t scale_min, scale_max, scale_step, window, slack, r_slack; /* as ucfp_panako_match_config */
    uint32_t bins;                                                     /* 0 = kept, 1 = scaled */
    uint32_t f_slack;                                                  /* 0 ... 3 bins; 0 when bins = 0 */
} ucfp_panako_match_config_ex;
int ucfp_panako_index_query_ex(ucfp_panako_index* ix, uint32_t tenant, const uint8_t* records, const uint64_t* offsets,
                               size_t nq, uint32_t k, uint32_t min_votes, const ucfp_panako_match_config_ex* cfg,
                               uint64_t* out_ids, uint32_t* out_votes, int32_t* out_offsets, uint32_t* out_scales,
                               float* out_scores, uint32_t* out_n);
int ucfp_panako_index_query_ex_dev(ucfp_panako_index* ix, uint32_t tenant, const uint8_t* d_records, const uint64_t* d_offsets,
                                   size_t nq, uint32_t k, uint32_t min_votes, const ucfp_panako_match_config_ex* cfg,
                                   uint64_t* d_out_ids, uint32_t* d_out_votes, int32_t* d_out_offsets, uint32_t* d_out_scales,
                                   float* d_out_scores, uint32_t* d_out_n, void* stream);

/* ---- Haitsma-Kalker sub-fingerprint index (the reference has no audio matcher) ----
 * A record r is a sequence F_r[0 .. n_r) of u32 sub-fingerprints (the bytes of an audiofp-haitsma-v1 record, 4 per
 * frame, little endian); a query is a sequence Q[0 .. m), m <= UCFP_HAITSMA_MAX_QUERY_FRAMES.  Item i of a batch is
 * frames[offsets[i] .. offsets[i+1]) with ELEMENT offsets (frames): offsets[0] = 0, non-decreasing, n + 1 entries --
 * the shape ucfp_audio_haitsma_batch_dev writes as d_out_offsets.
 * Within a tenant, P(v) = positions (r, t) with F_r[t] == v; an index with max_postings > 0 stops every v with
 * P(v) > max_postings (0 = no cap).  An alignment (r, d) is admissible iff 0 <= d and d + m <= n_r; it is a candidate
 * iff some j < m has popcount(F_r[d+j] ^ Q[j]) <= flip_bits with F_r[d+j] not stopped (flip_bits 0, 1 or 2: 1, 33 or
 * 529 probe values per query frame).  dist(r, d) = sum over j of popcount(F_r[d+j] ^ Q[j]); dist(r) = the minimum over
 * the candidates of r, offset(r) = the smallest d attaining it (the position of the query's frame 0 in the record).
 * Hits: dist(r) * 1000000 <= max_ber_ppm * 32 * m in 64-bit integers (max_ber_ppm <= 1000000), ordered (dist asc,
 * id asc), first k <= UCFP_INDEX_MAX_K; score = 1.0f - (float)dist / (float)(32 * m).  Unused output slots: id
 * UINT64_MAX, dist UINT32_MAX, offset 0, score -1.  k = 0, m = 0 or an unknown / empty tenant gives 0 hits; bad offsets,
 * m > UCFP_HAITSMA_MAX_QUERY_FRAMES, flip_bits > 2 or max_ber_ppm > 1000000 give UCFP_E_INVALID before anything runs.
 * Upsert of a known id replaces its frames, delete removes it, a record with 0 frames counts in `size`; postings are
 * rebuilt lazily at the next query, size or flush of a changed tenant.  Limits: a record below 2^31 frames, a tenant
 * below 2^32 - 1 frames in all, one query below 2^32 - 1 seeds (positions its probes find).  Queries read the checked
 * sizes back to the host once and the seed count of each query once per pass of 1024 queries (synchronisations of
 * `stream`) to size their buffers; queries whose seeds exceed the workspace are processed in slices, with the same
 * answers.  upsert_dev copies
 * its inputs to the host record table (it synchronises `stream`).  flags: 0. */
#define UCFP_HAITSMA_MAX_QUERY_FRAMES 4096u
typedef struct ucfp_haitsma_index ucfp_haitsma_index;
/* probe values per query frame: 1, 33, 529 for flip_bits 0, 1, 2; 0 for anything else.  Host only. */
size_t ucfp_haitsma_index_probes(uint32_t flip_bits);
int ucfp_haitsma_index_create(ucfp_ctx* ctx, uint32_t max_postings, uint32_t flags, ucfp_haitsma_index** out);
void ucfp_haitsma_index_destroy(ucfp_haitsma_index* ix);
int ucfp_haitsma_index_upsert(ucfp_haitsma_index* ix, uint32_t tenant, const uint64_t* ids, const uint32_t* frames,
                              const uint64_t* offsets, size_t n);
int ucfp_haitsma_index_upsert_dev(ucfp_haitsma_index* ix, uint32_t tenant, const uint64_t* d_ids, const uint32_t* d_frames,
                                  const uint64_t* d_offsets, size_t n, void* stream);
int ucfp_haitsma_index_delete(ucfp_haitsma_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed);
/* records = live records (empty ones included); frames = their frames in all (rebuilds a changed tenant). */
int ucfp_haitsma_index_size(ucfp_haitsma_index* ix, uint32_t tenant, size_t* records, size_t* frames);
int ucfp_haitsma_index_flush(ucfp_haitsma_index* ix);
/* nq ragged queries; out_ids / out_dist / out_offsets / out_scores are nq x k; out_n[q] = hits of query q. */
int ucfp_haitsma_index_query(ucfp_haitsma_index* ix, uint32_t tenant, const uint32_t* frames, const uint64_t* offsets,
                             size_t nq, uint32_t k, uint32_t flip_bits, uint32_t max_ber_ppm, uint64_t* out_ids,
                             uint32_t* out_dist, int32_t* out_offsets, float* out_scores, uint32_t* out_n);
int ucfp_haitsma_index_query_dev(ucfp_haitsma_index* ix, uint32_t tenant, const uint32_t* d_frames, const uint64_t* d_offsets,
                                 size_t nq, uint32_t k, uint32_t flip_bits, uint32_t max_ber_ppm, uint64_t* d_out_ids,
                                 uint32_t* d_out_dist, int32_t* d_out_offsets, float* d_out_scores, uint32_t* d_out_n,
                                 void* stream);

/* STREAMING Haitsma: the input side of continuous monitoring, with the state on the device and many
 * streams advanced by one push.  A set holds max_streams slots; a slot is one stream at the set's sample rate (1 000 ..
 * 384 000 Hz, resampled to 5 kHz like ucfp_audio_haitsma unless it is 5000).  The Haitsma spec is local in time: frame f
 * depends on 2048 samples at 5 kHz and on the band energies of frame f - 1.  After a push that brings a stream to n
 * samples it has emitted its first Fr(n) sub-fingerprints (ucfp_haitsma_stream_frames), a final push emits the rest, and
 * the concatenation over all pushes equals ucfp_audio_haitsma of the whole stream byte for byte, however the stream is
 * cut into chunks (empty chunks and a final push without samples included).  Frame 0 of a stream has a zero history;
 * every later frame uses the energies of the frame before it, also across pushes.
 *   - The set serialises its own calls: it is safe to call from several threads.  Consecutive calls are ordered by the
 *     set itself (an event), whatever `stream` the caller passes.
 *   - Device bytes per stream: ucfp_haitsma_streams_state_bytes(sample_rate, block_frames) =
 *     4 * (2048 + ceil(sample_rate / 5000) + 1 + 33 + block_frames): the 5 kHz tail of the next frame, the input samples
 *     the next output still needs, the last frame's band energies and the ring of the latest block_frames
 *     sub-fingerprints; fixed at creation, whatever the stream's length.  The push path allocates nothing beyond growing
 *     the context's workspace to the largest push seen.
 *   - Errors are status codes: UCFP_E_INVALID for a slot out of range or not open, a slot twice in one call, a chunk
 *     above 2^29 samples, a push whose carried plus new 5 kHz samples reach 2^31, a stream that would pass 2^32 frames,
 *     block_frames above UCFP_HAITSMA_MAX_QUERY_FRAMES, cap_frames below the bound; UCFP_E_MODALITY for a rate outside
 *     1 000 .. 384 000 or band edges outside 1 <= fmin < fmax <= 2500.  A failed call changes no state. */
typedef struct ucfp_haitsma_streams ucfp_haitsma_streams;
/* cfg as ucfp_audio_haitsma, NULL = defaults.  The rate and the band edges are checked before anything else.
 * block_frames in [0, UCFP_HAITSMA_MAX_QUERY_FRAMES]: the length of the live block (0: no ring).  Fails with UCFP_E_INDEX
 * without a gfx950 device (no CPU fallback). */
int ucfp_haitsma_streams_create(ucfp_ctx* ctx, uint32_t sample_rate, const ucfp_haitsma_config* cfg, uint32_t max_streams,
                                uint32_t block_frames, ucfp_haitsma_streams** out);
void ucfp_haitsma_streams_destroy(ucfp_haitsma_streams* s);
int ucfp_haitsma_streams_open(ucfp_haitsma_streams* s, uint32_t* slot);     /* fresh stream: no samples, zero history */
int ucfp_haitsma_streams_close(ucfp_haitsma_streams* s, uint32_t slot);     /* discard, emit nothing */
/* Host-only, no GPU: Fr of A18 -- S(n) = n at 5 kHz, else min(ceil((n - 1) 5000 / sr), floor(n 5000 / sr)) (S(0) = 0;
 * final: floor(n 5000 / sr)); Fr = S < 2048 ? 0 : (S - 2048) / 64 + 1.  0 for a rate outside 1 000 .. 384 000. */
uint64_t ucfp_haitsma_stream_frames(uint64_t n_samples, uint32_t sample_rate, int final);
/* Host-only: device bytes a set holds per stream (0 for a rate or block_frames out of range). */
size_t ucfp_haitsma_streams_state_bytes(uint32_t sample_rate, uint32_t block_frames);
/* The frames a push emits, exactly; host-computable from the per-slot sample counts (0 for an invalid push). */
size_t ucfp_haitsma_streams_max_frames(ucfp_haitsma_streams* s, const uint32_t* slots, const uint64_t* n_samples,
                                       const uint8_t* final, size_t n);
/* slots / n_samples / final: host arrays of n entries (distinct open slots; final may be NULL = none); d_pcm: the n
 * chunks concatenated in that order on the device.  Sub-fingerprints of entry i -> d_out[d_out_offsets[i] ..
 * d_out_offsets[i+1]) (u32 each; n + 1 device u64 offsets).  final[i] != 0 emits the rest and closes the slot.
 * cap_frames below ucfp_haitsma_streams_max_frames -> UCFP_E_INVALID before ANY state changes.  One launch sequence
 * whatever n is; no host synchronisation (the host waits only for the table copy of the call two back). */
int ucfp_haitsma_streams_push_dev(ucfp_haitsma_streams* s, const uint32_t* slots, const uint64_t* n_samples,
                                  const uint8_t* final, size_t n, const float* d_pcm, uint32_t* d_out, size_t cap_frames,
                                  uint64_t* d_out_offsets, void* stream);
/* Host-pointer convenience for one slot; synchronous.  *n_frames = frames of this push. */
int ucfp_haitsma_streams_push(ucfp_haitsma_streams* s, uint32_t slot, const float* pcm, size_t n, int final, uint32_t* out,
                              size_t cap_frames, size_t* n_frames);
/* Live blocks: item i = the latest min(block_frames, frames emitted) sub-fingerprints of open slot slots[i] in time
 * order -> d_frames[d_offsets[i] .. d_offsets[i+1]) (element offsets, n + 1 of them): the ragged shape
 * ucfp_haitsma_index_query_dev takes.  A stream without frames gives an empty item.  cap_frames below the total ->
 * UCFP_E_INVALID.  No host synchronisation. */
int ucfp_haitsma_streams_blocks_dev(ucfp_haitsma_streams* s, const uint32_t* slots, size_t n, uint32_t* d_frames,
                                    size_t cap_frames, uint64_t* d_offsets, void* stream);

/* ---- BM25 keyword index (src/index/embedded/bm25.rs:79-628) ----
 * A document is a list of (key u64, tf u32) pairs: item i of a batch is keys/tfs[offsets[i] .. offsets[i+1]) with
 * ELEMENT offsets (offsets[0] = 0, non-decreasing, n + 1 entries); dl = sum tf < 2^32.  Keys are the caller's: equal
 * terms of a tenant must map to equal keys (the Python mirror numbers its terms; the Rust host can pass FST term ids).
 * A key twice in one document, tf = 0 or bad offsets give UCFP_E_INVALID before anything changes.  A document without
 * pairs still counts in N.  Upsert of a known id replaces the document, delete removes it; postings are rebuilt lazily
 * at the next query or flush of a changed tenant.
 * A query is a list of keys (order and duplicates kept; an unknown key matches nothing).  With N live documents,
 * T = sum dl, avgdl = (float)T / (float)N, df_j = documents holding key j, idf_j = logf((N - df_j + 0.5f) /
 * (df_j + 0.5f) + 1.0f) by the HOST's logf, c = (idf_j * (tf * (K1 + 1))) / fmaxf(tf + K1 * ((1 - B) + (B * dl) /
 * fmaxf(avgdl, 1)), 1e-6f) with K1 = 1.2f, B = 0.75f, all f32 one operation at a time; score = sum of c in key order
 * from 0.  Hits: every document holding some query key, ordered (score desc, id asc), first k <= UCFP_INDEX_MAX_K.
 * Unused output slots: id UINT64_MAX, score -1.  k = 0, an empty query or an unknown / empty tenant gives 0 hits.
 * Optional explain outputs (NULL = not written): out_idf[offsets[q] + j] = idf of position j (0 for an unknown key);
 * out_tf / out_contrib[k * offsets[q] + h * m_q + j] = tf and c of hit h at position j of query q (m_q keys; 0 when the
 * hit does not hold the key or h >= out_n[q]).  A query reads df of its keys back to the host once (one synchronisation
 * of `stream`; query_dev also reads the offsets); the rest is asynchronous.  A query with more than
 * UCFP_BM25_LDS_POSTINGS postings in all is scored by ordinal ranges instead of in one LDS table; both give the same
 * bits.  upsert_dev copies its inputs to the host document table (it synchronises `stream`).  flags: 0. */
#define UCFP_BM25_LDS_POSTINGS 6144u
typedef struct ucfp_bm25_index ucfp_bm25_index;
int ucfp_bm25_index_create(ucfp_ctx* ctx, uint32_t flags, ucfp_bm25_index** out);
void ucfp_bm25_index_destroy(ucfp_bm25_index* ix);
int ucfp_bm25_index_upsert(ucfp_bm25_index* ix, uint32_t tenant, const uint64_t* ids, const uint64_t* keys,
                           const uint32_t* tfs, const uint64_t* offsets, size_t n);
int ucfp_bm25_index_upsert_dev(ucfp_bm25_index* ix, uint32_t tenant, const uint64_t* d_ids, const uint64_t* d_keys,
                               const uint32_t* d_tfs, const uint64_t* d_offsets, size_t n, void* stream);
int ucfp_bm25_index_delete(ucfp_bm25_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed);
/* docs = live documents (empty ones included); postings = (key, document) pairs. */
int ucfp_bm25_index_size(ucfp_bm25_index* ix, uint32_t tenant, size_t* docs, size_t* postings);
int ucfp_bm25_index_flush(ucfp_bm25_index* ix);
/* nq ragged queries; out_ids / out_scores are nq x k; out_n[q] = hits of query q. */
int ucfp_bm25_index_query(ucfp_bm25_index* ix, uint32_t tenant, const uint64_t* keys, const uint64_t* offsets, size_t nq,
                          uint32_t k, uint64_t* out_ids, float* out_scores, uint32_t* out_n, float* out_idf,
                          uint32_t* out_tf, float* out_contrib);
int ucfp_bm25_index_query_dev(ucfp_bm25_index* ix, uint32_t tenant, const uint64_t* d_keys, const uint64_t* d_offsets,
                              size_t nq, uint32_t k, uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_out_n,
                              float* d_out_idf, uint32_t* d_out_tf, float* d_out_contrib, void* stream);

/* ---- BM25 terms: tokenise, hash and count on the device (bm25.rs:88-97 `tokenize`, :343) ----
 * Document i of a batch is utf8[offsets[i] .. offsets[i+1]) (BYTE offsets, n + 1 entries).  A token is a maximal run of
 * bytes in [0-9A-Za-z] with A-Z mapped to a-z; every other byte separates ('_', '\'', '.', ':', ',' and ';' included:
 * this is not the word rule of the MinHash / SimHash entries).  Its key is XXH3_64 of the lower-cased bytes, seed 0 =
 * ucfp_text_token_key.  Every u64 is a legal key; two terms whose keys collide are one term.
 *   form UCFP_BM25_TERMS_COUNTS    the distinct keys of each document in ascending order, each with its count tf: what
 *                                  ucfp_bm25_index_upsert(_dev) takes (a key never twice in one document);
 *        UCFP_BM25_TERMS_SEQUENCE  one key per token in text order, duplicates kept: what ucfp_bm25_index_query(_dev)
 *                                  takes.  tfs is not written and may be NULL.
 * Document i's pairs are keys/tfs[pair_offsets[i] .. pair_offsets[i+1]): ELEMENT offsets, n + 1 entries, non-decreasing,
 * pair_offsets[0] = 0.  status[i]:
 *   0                     every ASCII document; one of length 0 or without a letter or digit has no pairs (it still
 *                         counts in N of the index);
 *   UCFP_TEXT_NEEDS_HOST  a byte >= 0x80 anywhere in the document: no pairs, and this status wins.  Unicode
 *                         is_alphanumeric and to_lowercase (Final_Sigma, U+0130) stay on the host;
 *   UCFP_E_UNSUPPORTED    only for a document holding a token of more than UCFP_TEXT_MAX_WINDOW_BYTES bytes: no pairs.
 *                         Tokens up to that length are never refused; above it the document gets either status 0 and the
 *                         right pairs or this status;
 *   UCFP_E_INVALID        offsets[i+1] < offsets[i], offsets[i+1] > n_bytes, offsets[i] below an earlier offset of the
 *                         table (the document would share bytes with an earlier one) or 2^31 bytes and more: no pairs.
 *                         No byte outside [0, n_bytes) is read.
 * A document whose status is not 0 has an empty range.  cap_pairs >= ucfp_bm25_terms_max_pairs(n_bytes, n) = (n_bytes +
 * n) / 2 (host-only): a token takes a byte and two tokens a separator between them.  The host form takes n_bytes =
 * offsets[n].  UCFP_E_INVALID before anything runs or is written: ctx NULL (checked first), an unknown form, a NULL
 * buffer (tfs in form COUNTS; utf8 when n_bytes > 0), n >= 2^31, n_bytes + n >= 2^33, cap_pairs below the bound.
 * The scratch (6 bytes per input byte, 28 per token in form COUNTS) belongs to the context and grows on demand; calls
 * on different streams are ordered on the device.  HOST SYNCHRONISATIONS of the _dev form: SEQUENCE none; COUNTS one of
 * `stream`, to read the batch's token count back (it sizes the sort).  A call that grows the scratch frees the old
 * buffers, which waits for the device. */
#define UCFP_BM25_TERMS_COUNTS 0
#define UCFP_BM25_TERMS_SEQUENCE 1
size_t ucfp_bm25_terms_max_pairs(size_t n_bytes, size_t n);
int ucfp_bm25_terms_batch_dev(ucfp_ctx* ctx, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, size_t n_bytes,
                              int form, uint64_t* d_keys, uint32_t* d_tfs, size_t cap_pairs, uint64_t* d_pair_offsets,
                              int32_t* d_status, void* stream);
int ucfp_bm25_terms_batch(ucfp_ctx* ctx, const uint8_t* utf8, const uint64_t* offsets, size_t n, int form, uint64_t* keys,
                          uint32_t* tfs, size_t cap_pairs, uint64_t* pair_offsets, int32_t* status);

/* =============================== INDEX ========================================
 * Replaces `trait IndexBackend` kNN (src/index/mod.rs:29-35) as implemented by
 * EmbeddedBackend::knn (src/index/embedded/mod.rs:268-360): exact brute-force top-k inside
 * one tenant.  COSINE_F32 is the reference's kernel (dot_product :454-472, l2_norm :475-477,
 * insert_topk :484-495); HAMMING64 is the new capability BASELINE config 5 asks for behind
 * /v1/query (the reference has no Hamming search: SURVEY F3).  redb stays the source of
 * truth on the Rust side; this object is the GPU-resident mirror of one shard.
 *
 * Ordering: best first; ties broken by ascending record_id (the reference leaves tie order to
 * rayon's split, i.e. unspecified).  Hamming: distance d = popcount(q ^ x), score = 1 - d/64
 * so that "higher is better" holds (src/core/mod.rs:113-115).  Cosine: score =
 * dot/(|q||v|); zero-norm rows are skipped, a zero-norm query yields no hits (:283-286,:328-330).
 * Every reported cosine score is an f32 dot product; where a batch is steered by f16 matrix-core arithmetic (the chunk
 * minima of 2 .. 64 queries per pass, round 4) that arithmetic only selects WHICH chunks of rows get their exact scores
 * computed, under a proven error bound -- it never reaches an answer.
 */
typedef struct ucfp_index ucfp_index;

typedef enum ucfp_index_kind {
    UCFP_INDEX_HAMMING64 = 1, /* rows are uint64_t                                   */
    UCFP_INDEX_COSINE_F32 = 2 /* rows are float[dim]                                 */
} ucfp_index_kind;

#define UCFP_INDEX_APPEND_ONLY 1u /* no id->row map: upsert appends, delete unsupported   */
#define UCFP_INDEX_MAX_K 128u      /* web caps k at 100 (web/src/routes/api/search/+server.ts:11) */
#define UCFP_INVALID_ID 0xffffffffffffffffull

int ucfp_index_create(ucfp_ctx* ctx, int kind, uint32_t dim, uint32_t flags, ucfp_index** out);
void ucfp_index_destroy(ucfp_index* idx);

/* IndexBackend::upsert (src/index/mod.rs:20-22): rows with a known id are overwritten in
 * place, new ids are appended to the tenant's contiguous range. Host pointers. */
int ucfp_index_upsert(ucfp_index* idx, uint32_t tenant, const uint64_t* ids, const void* rows, size_t n);
/* Bulk append of device-resident rows (APPEND_ONLY indexes; corpus loaders, benches). */
int ucfp_index_append_dev(ucfp_index* idx, uint32_t tenant, const uint64_t* d_ids, const void* d_rows,
                          size_t n, void* stream);
/* IndexBackend::delete (src/index/mod.rs:24-27). `n_removed` may be NULL. */
int ucfp_index_delete(ucfp_index* idx, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed);
int ucfp_index_size(ucfp_index* idx, uint32_t tenant, size_t* out);
/* IndexBackend::flush (src/index/mod.rs:63): waits for queued device work. */
int ucfp_index_flush(ucfp_index* idx);
/* Snapshot of the device mirror (the sidecar flat file GPU shards are rebuilt from at start-up; redb,
 * `src/index/embedded/mod.rs:37-43,104-125`, stays the reference's source of truth).  `load` upserts the
 * snapshot's rows into an index of the same kind / dim. */
int ucfp_index_save(ucfp_index* idx, const char* path);
int ucfp_index_load(ucfp_index* idx, const char* path);

/* IndexBackend::knn for a batch of queries (nq = 1 is the reference's call).
 *   queries     nq rows of the index kind (host memory)
 *   out_ids     nq x k   record ids, UCFP_INVALID_ID past out_counts[q]
 *   out_scores  nq x k   f32 score (higher is better)
 *   out_dist    nq x k   Hamming distance (HAMMING64 only; may be NULL)
 *   out_counts  nq       hits returned for each query (<= k)
 * An unknown tenant or k = 0 returns zero hits, like the reference (:275-277). */
int ucfp_index_search(ucfp_index* idx, uint32_t tenant, const void* queries, size_t nq, uint32_t k,
                      uint64_t* out_ids, float* out_scores, uint32_t* out_dist, uint32_t* out_counts);
/* Same with device pointers, enqueued on `stream` (no synchronisation).  Searches enqueued on different streams are ordered
 * only where they share a workspace: a HAMMING64 index alternates between two, so two batches may be in flight at once
 * (the short staging kernels of one run under the matrix-core scan of the other); cosine searches run one at a time.
 * COSINE_F32: any 4-byte-aligned d_queries pointer is accepted; a pointer that is not 16-byte aligned costs one device copy. */
int ucfp_index_search_dev(ucfp_index* idx, uint32_t tenant, const void* d_queries, size_t nq, uint32_t k,
                          uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_out_dist,
                          uint32_t* d_out_counts, void* stream);

/* Filtered search (DESIGN F1 - F6): `Query.filter` (src/core/mod.rs:165-167), a set of record ids as the portable
 * serialization of a 64-bit Roaring treemap (what RoaringTreemap::serialize_into writes).  A filter becomes a VIEW of one
 * (index, tenant): a compact sub-shard of the allowed rows, in the shard's row order, that the Hamming and cosine searches
 * read exactly as they read a shard -- a filtered search answers, bit for bit, what an index holding only the allowed rows
 * answers.  Malformed bytes are UCFP_E_INVALID with the byte offset in ucfp_last_error().
 *
 * ucfp_roaring_validate: host only, no context; `cardinality` (may be NULL) = ids in the set.
 * ucfp_index_filter_create: one call, one host synchronisation (the allowed-row count sizes the view).  An unknown tenant or
 *   an empty filter gives a view of 0 rows.  The view keeps a copy of the bytes.
 * ucfp_index_filter_stale: 1 once the tenant's shard changed since the view was built (upsert, append_dev, delete, load),
 *   0 while it is current, UCFP_E_INVALID for a NULL or detached view.  ucfp_index_filter_refresh rebuilds it.
 * ucfp_index_filter_stats: rows in the view, rows of the shard it was built from, containers of the filter, device bytes
 *   it holds (any pointer may be NULL).
 * Destroying the index first detaches its views: every later call on them but destroy returns UCFP_E_INVALID.
 * Refreshing a view that holds rows and destroying a view synchronise the whole device (a search on any stream may still
 * read the buffers they free).
 * A view lives in device memory (rows_allowed x (8 + row bytes [+ 4 cosine]) + the filter's image + 16 bytes per 64 shard
 * rows) until it is destroyed; views are not part of ucfp_index_save. */
typedef struct ucfp_index_filter ucfp_index_filter;
int ucfp_roaring_validate(const uint8_t* bytes, size_t len, uint64_t* cardinality);
int ucfp_index_filter_create(ucfp_index* idx, uint32_t tenant, const uint8_t* bytes, size_t len, ucfp_index_filter** out);
void ucfp_index_filter_destroy(ucfp_index_filter* f);
int ucfp_index_filter_stats(ucfp_index_filter* f, size_t* rows_allowed, size_t* rows_seen, size_t* containers,
                            size_t* device_bytes);
/* Milliseconds of the view's last build on the device (0 for a view of 0 rows; any pointer may be NULL): the probe, the scan
 * of the tile counts, from the end of the scan to the start of the gather (the read-back of the row count, the host's
 * wake-up and the allocation of the view), and the gather with the ids-ascend pass. */
int ucfp_index_filter_build_ms(ucfp_index_filter* f, float* probe_ms, float* scan_ms, float* readback_ms, float* gather_ms);
/* Self-check for tests: every buffer of a view lies between 256-byte guard patterns (its mask / count scratch has one
 * behind it); synchronises the device and returns UCFP_E_INDEX, naming the buffer, if a guard was overwritten. */
int ucfp_index_filter_check(ucfp_index_filter* f);
int ucfp_index_filter_stale(ucfp_index_filter* f);
int ucfp_index_filter_refresh(ucfp_index_filter* f);
/* ucfp_index_search_dev / ucfp_index_search over a view: same arguments, checks, outputs and stream protocol.  A view of
 * another index is UCFP_E_INVALID.  The _dev entry refuses a stale view (UCFP_E_INVALID); the host entry refreshes it. */
int ucfp_index_search_filtered_dev(ucfp_index* idx, ucfp_index_filter* f, const void* d_queries, size_t nq, uint32_t k,
                                   uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_out_dist,
                                   uint32_t* d_out_counts, void* stream);
int ucfp_index_search_filtered(ucfp_index* idx, ucfp_index_filter* f, const void* queries, size_t nq, uint32_t k,
                               uint64_t* out_ids, float* out_scores, uint32_t* out_dist, uint32_t* out_counts);

/* Multi-tenant search (DESIGN M1 - M6): one batch for the queries of many tenants.  Every shape of the reference carries a
 * tenant_id (src/core/mod.rs) and the requests in flight belong to whatever tenants are calling; the entries above take one
 * tenant per call, so the queries of ten thousand small tenants are ten thousand chains of launches.  Here query i searches
 * tenant tenants[i]; the number of launches does not depend on the tenants of the batch (hamming_multi.hip).
 *   tenants     nq tenant ids, HOST memory in both forms (the host owns the tenant -> shard map); read before the call returns
 *   outputs     the layout of ucfp_index_search[_dev]: nq x k (d_out_scores / d_out_dist may be NULL), counts nq
 * Row i of every output is, bit for bit, what ucfp_index_search_dev(idx, tenants[i], &query_i, 1, k, ...) writes: ids, score
 * bits, distances, the count and the padding past it, in (distance, record id) order.  An unknown tenant or one without
 * rows gives count 0 and a padded row; k = 0 zeroes the counts and writes nothing else; nq = 0 is UCFP_OK.  Tenants may
 * repeat, come in any order, and all be the same; a query's answer does not depend on the rest of the batch.
 * Checks: those of ucfp_index_search, and tenants == NULL with nq > 0 -> UCFP_E_INVALID.  HAMMING64 only: a COSINE_F32
 * index is UCFP_E_UNSUPPORTED, and filter views are not accepted.  A batch runs in chunks of 16 384 queries; a chunk whose
 * work items (ucfp_index_search_multi_limits: tiles of tile_rows rows x chunks of query_chunk queries, per tenant) number
 * more than (2^32 - 1) / 256, or a batch that names a tenant of more than 2^32 - 1 rows, is UCFP_E_UNSUPPORTED before
 * anything runs.  Nothing is written on a refusal.
 * Each tenant's rows are read twice: a tenant with many rows AND many queries is better served by ucfp_index_search_dev.
 * The _dev form follows the stream protocol of ucfp_index_search_dev (a workspace slot, ordered against mutations) and has
 * ONE host wait: the pinned staging of the slot's plan tables is rewritten by the host, which first waits for the search
 * that used the slot last -- the search two calls back; none in the first two calls.  It synchronises nothing else.  That
 * wait is taken with the index's mutex held (the plan holds shard pointers that a mutation may free): while it lasts, other
 * threads' searches and mutations of this index queue behind it, as they do behind the synchronising mutations.
 * ucfp_index_search_multi_limits: host only; the constants of the implementation -- rows per work item, queries per work
 * item, ids of a query's tie list (more ties at the k-th distance take a gated exact pass); any pointer may be NULL. */
int ucfp_index_search_multi_dev(ucfp_index* idx, const uint32_t* tenants, const void* d_queries, size_t nq, uint32_t k,
                                uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_out_dist, uint32_t* d_out_counts,
                                void* stream);
int ucfp_index_search_multi(ucfp_index* idx, const uint32_t* tenants, const void* queries, size_t nq, uint32_t k,
                            uint64_t* out_ids, float* out_scores, uint32_t* out_dist, uint32_t* out_counts);
int ucfp_index_search_multi_limits(uint32_t* tile_rows, uint32_t* query_chunk, uint32_t* tie_cap);

/* Host micro-batcher for the QUERY route: /v1/query is one query per request (src/server/handlers.rs:143-187),
 * up to 512 requests in flight (src/bin/ucfp.rs:267).  submit() is BLOCKING and thread-safe: concurrent calls -- each with
 * ITS OWN query (a u64 hash, or dim floats) and ITS OWN k (QueryRequest.k, src/server/dto.rs:74-87) -- become ONE copy of the
 * queries + ONE ucfp_index_search_dev with the largest k of the batch + one copy of the results; a request gets the first k
 * entries of its row (the order is total: (distance, id) / (score desc, id)).  One batcher per (index, tenant); at most
 * max_batch (<= 4096) queries per flush, flushed no later than max_delay_us after the first pending query.  (All batchers:
 * behind a flush that carried several requests the next one waits up to 10 us -- or until as many requests have arrived
 * as that flush carried -- even with max_delay_us = 0: its submitters are on their way back with their next request.  A
 * lone sequential client is flushed at once.)
 *   out_ids / out_scores / out_dist   k entries each (scores, dist may be NULL); places past *out_count carry
 *                                     UCFP_INVALID_ID / -1 / 2^32 - 1 like ucfp_index_search. */
typedef struct ucfp_search_batcher ucfp_search_batcher;
int ucfp_index_search_batcher_create(ucfp_index* idx, uint32_t tenant, size_t max_batch, uint32_t max_delay_us,
                                     ucfp_search_batcher** out);
void ucfp_index_search_batcher_destroy(ucfp_search_batcher* b);
int ucfp_index_search_batcher_submit(ucfp_search_batcher* b, const void* query, uint32_t k, uint64_t* out_ids, float* out_scores,
                                     uint32_t* out_dist, uint32_t* out_count);
int ucfp_index_search_batcher_stats(ucfp_search_batcher* b, uint64_t* batches, uint64_t* items);
/* The same object for the requests of MANY tenants (DESIGN M5): one batcher per index, every submit names its tenant, one
 * flush is ONE ucfp_index_search_multi_dev with the largest k of the batch.  Limits, flush rules, stats and destroy as above.
 * ucfp_index_search_batcher_submit on a multi batcher and ucfp_index_search_batcher_submit_tenant on a per-tenant one are
 * UCFP_E_INVALID; create_multi on a COSINE_F32 index is UCFP_E_UNSUPPORTED. */
int ucfp_index_search_batcher_create_multi(ucfp_index* idx, size_t max_batch, uint32_t max_delay_us, ucfp_search_batcher** out);
int ucfp_index_search_batcher_submit_tenant(ucfp_search_batcher* b, uint32_t tenant, const void* query, uint32_t k,
                                            uint64_t* out_ids, float* out_scores, uint32_t* out_dist, uint32_t* out_count);

/* Final step of a sharded search: merge `parts` per-shard top-k lists -- the
 * all-gathered [parts][nq][k] ids + keys -- into one. Keys: Hamming distance (kind
 * HAMMING64) or the order-preserving u32 image of -score (COSINE_F32) as produced by
 * ucfp_index_search_dev in d_out_dist. Device pointers.
 * The answer is the best k by (key, id) ascending, both unsigned; an entry with key 2^32-1 is no entry wherever it
 * stands in its list.  Equal (key, id) pairs from different parts (a stale row that lives in two shards) are emitted
 * ONCE; the same id under two different keys is two entries.  Any number of parts. */
int ucfp_topk_merge_dev(ucfp_ctx* ctx, int kind, const uint64_t* d_part_ids, const uint32_t* d_part_keys,
                        uint32_t parts, size_t nq, uint32_t k, uint64_t* d_out_ids, float* d_out_scores,
                        uint32_t* d_out_keys, uint32_t* d_out_counts, void* stream);

/* ---- the packed wire format of a sharded search: 16-byte entries {u64 id, u32 key, u32 0}, [nq][k] per shard.
 * For hosts that move the per-shard lists with their own transport (MPI, gloo, host TCP) instead of RCCL:
 * pack -> (their all-gather into [parts][nq][k] entries) -> merge_packed. */
int ucfp_topk_pack_dev(ucfp_ctx* ctx, const uint64_t* d_ids, const uint32_t* d_keys, size_t nq, uint32_t k,
                       void* d_entries, void* stream);
/* The same merge and the same rule as ucfp_topk_merge_dev (equal (key, id) pairs from different parts are emitted once).
 * Limits: parts <= 64, or any number of parts while parts * k <= 2048; beyond that UCFP_E_UNSUPPORTED. */
int ucfp_topk_merge_packed_dev(ucfp_ctx* ctx, int kind, const void* d_entries, uint32_t parts, size_t nq, uint32_t k,
                               uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_out_keys, uint32_t* d_out_counts,
                               void* stream);
/* The same with the missing-shard mask: a shard that could not scan sends nq x k entries of 0xff bytes (id 2^64-1, key
 * 2^32-1 like an empty list, and the pad word 0xffffffff where ucfp_topk_pack_dev writes 0); bit p of *d_missing (device
 * u64, may be NULL) is set for every such part.  With a mask parts <= 64 always (one bit per part), also where the
 * merge alone would take more: UCFP_E_UNSUPPORTED otherwise. */
int ucfp_topk_merge_packed_ex_dev(ucfp_ctx* ctx, int kind, const void* d_entries, uint32_t parts, size_t nq, uint32_t k,
                                  uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_out_keys, uint32_t* d_out_counts,
                                  uint64_t* d_missing, void* stream);

/* ============================ SHARDED SEARCH (multi-GPU) ==============================
 * "Multi-GPU variant takes a device list; shards are internal" of IndexBackend::knn
 * (src/index/mod.rs:29-35).  Model: ONE PROCESS PER GPU (the "device list" is the job's ranks: rank r owns GPU
 * LOCAL_RANK and one ucfp_index holding its range of the corpus, ucfp_shard_range).  Queries are replicated; each
 * rank scans its shard; the only data-path exchange is ONE ncclAllGather (RCCL over xGMI) of the per-shard top-k
 * as packed 16-byte entries -- nq x k x 16 B per rank, latency-bound -- then every rank runs the same merge
 * ((key asc, id asc)) and holds the full answer.  The reference has no multi-device search.
 *
 *   rank 0:      ucfp_shard_unique_id(uid)            and ships the 128 bytes to the other ranks (the host's own
 *                                                     control channel: env, file, TCP -- like ncclUniqueId)
 *   every rank:  ucfp_shard_comm_create(ctx, uid, rank, world, &comm)     (collective: all ranks call it)
 *                ucfp_index_search_sharded_dev(idx, comm, ...)            (collective, same nq / k everywhere)
 * world = 1 needs no uid and never loads RCCL.  RCCL is dlopen()ed (librccl.so.1) when world > 1.
 *
 * ucfp_shard_comm_create_ex(..., flags, ...): UCFP_SHARD_FORCE_RCCL (or UCFP_SHARD_FORCE_RCCL=1 in the environment)
 * builds a real RCCL communicator even at world = 1 (uid required) -- ncclCommInitRank(nranks = 1), one ncclAllGather
 * per batch on the exchange stream, the merge over the gathered buffer -- so that a single-GPU host executes, and can
 * test, exactly the code path a multi-GPU job runs.  ucfp_shard_comm_uses_rccl tells which branch a communicator takes.
 *
 * Failure of one rank: if this rank's own shard scan cannot be enqueued (or any later local step fails),
 * ucfp_index_search_sharded_submit still joins the all-gather with an empty list (so the other ranks do not block),
 * completes the ticket and returns the error; the answer every rank then holds lacks that shard, and every rank can tell:
 * the list carries a mark in the entries' pad word that the merge turns into ucfp_index_search_sharded_missing's mask. */
#define UCFP_SHARD_UID_BYTES 128
#define UCFP_SHARD_FORCE_RCCL 1u
typedef struct ucfp_shard_comm ucfp_shard_comm;
int ucfp_shard_unique_id(uint8_t uid[UCFP_SHARD_UID_BYTES]);
int ucfp_shard_comm_create(ucfp_ctx* ctx, const uint8_t uid[UCFP_SHARD_UID_BYTES], int rank, int world,
                           ucfp_shard_comm** out);
int ucfp_shard_comm_create_ex(ucfp_ctx* ctx, const uint8_t uid[UCFP_SHARD_UID_BYTES], int rank, int world,
                              uint32_t flags, ucfp_shard_comm** out);
int ucfp_shard_comm_uses_rccl(ucfp_shard_comm* comm);   /* 1: batches go through ncclAllGather; 0: local short cut */
void ucfp_shard_comm_destroy(ucfp_shard_comm* comm);
/* rank / world / number of all-gathers issued so far (each may be NULL) */
int ucfp_shard_comm_info(ucfp_shard_comm* comm, int* rank, int* world, uint64_t* exchanges);
/* [start, end) of a corpus of n_total rows (global insertion order) owned by `rank`: contiguous ranges, the first
 * n_total % world ranks hold one extra row. */
void ucfp_shard_range(uint64_t n_total, int rank, int world, uint64_t* start, uint64_t* end);

/* Sharded IndexBackend::knn for a batch (device pointers; queries identical on every rank).
 * submit: the shard scan is enqueued BEHIND `stream` (whatever wrote the queries there has finished) on the scan stream of
 *         one of the communicator's two buffer sets, the all-gather + merge on its exchange stream: the scans of two
 *         successive batches run side by side (one's short staging kernels fill the gaps of the other's matrix-core
 *         scan) and the exchange of a batch overlaps the scan of the next; at most two batches in flight.
 *         Outputs (as ucfp_index_search_dev; d_out_scores / d_out_keys may be NULL) are written by those streams:
 *         they and the queries must stay untouched until the ticket is collected.
 * collect: makes `stream` wait for that batch's results (no host synchronisation).
 * ucfp_index_search_sharded_dev = submit + collect on the same stream. */
int ucfp_index_search_sharded_submit(ucfp_index* idx, ucfp_shard_comm* comm, uint32_t tenant, const void* d_queries,
                                     size_t nq, uint32_t k, uint64_t* d_out_ids, float* d_out_scores,
                                     uint32_t* d_out_keys, uint32_t* d_out_counts, void* stream, uint64_t* ticket);
int ucfp_index_search_sharded_collect(ucfp_shard_comm* comm, uint64_t ticket, void* stream);
/* Which shards are ABSENT from a ticket's answer: bit r of *missing_mask = rank r joined the all-gather with the empty list of
 * a failed scan (see "Failure of one rank" above) -- the same mask on every rank, so a host can report a partial result
 * wherever it reads the answer, not only on the rank that failed.  Waits for the batch (host synchronisation); valid while
 * the ticket's buffer set has not been handed to a later batch (i.e. before the second submit after it). */
int ucfp_index_search_sharded_missing(ucfp_shard_comm* comm, uint64_t ticket, uint64_t* missing_mask);
int ucfp_index_search_sharded_dev(ucfp_index* idx, ucfp_shard_comm* comm, uint32_t tenant, const void* d_queries,
                                  size_t nq, uint32_t k, uint64_t* d_out_ids, float* d_out_scores,
                                  uint32_t* d_out_keys, uint32_t* d_out_counts, void* stream);

/* ---- JPEG front end ----
 * The reference's image route also takes JPEG uploads (src/modality/image.rs:54 "PNG / JPEG / WebP / GIF / BMP", decoders at
 * Cargo.toml:143) and decodes them inside the same SDK call (image.rs:68-70, :176-179).  Same call shape as the PNG entry
 * points: one blob + n + 1 byte offsets, ONE announced geometry (ucfp_jpeg_probe reads it from the frame header).  What
 * is decoded of a JPEG is its LUMA component (DESIGN J1: the Y plane of a YCbCr file, the plane of a greyscale one; chroma
 * is parsed, never transformed): frames are GRAY8, and what libjpeg returns for out_color_space = JCS_GRAYSCALE with the
 * accurate integer IDCT, bit for bit.  One wave per file, one lane per restart interval (Huffman decoding is serial
 * within one), one thread per 8x8 block for the inverse DCT.  status[i]:
 *   0                      decoded (and hashed)
 *   UCFP_IMAGE_NEEDS_HOST  a JPEG this path does not decode (progressive, arithmetic-coded, 12-bit, CMYK / RGB-coded,
 *                          several scans, luma below the MCU's resolution, 16-bit quantisation tables), another geometry
 *                          than announced, or ANY irregularity of the entropy-coded data: the host's decoder decides
 *   UCFP_E_MODALITY        no SOI marker: not a JPEG (the reference answers 400)
 * jpg_bytes = d_offsets[n]; workspace about jpg_bytes + n x 3 x width x height bytes. */
int ucfp_jpeg_probe(const uint8_t* jpg, size_t len, uint32_t* width, uint32_t* height);
int ucfp_image_jpeg_decode_batch_dev(ucfp_ctx* ctx, const uint8_t* d_jpg, const uint64_t* d_offsets, size_t n,
                                     size_t jpg_bytes, uint32_t width, uint32_t height, uint8_t* d_frames,
                                     size_t row_stride, size_t frame_stride, int32_t* d_status, void* stream);
/* Encoded files -> records (as ucfp_image_png_hash_batch_dev; d_exact NULL: BLAKE3 of every file on the device). */
int ucfp_image_jpeg_hash_batch_dev(ucfp_ctx* ctx, uint32_t algo, const uint8_t* d_jpg, const uint64_t* d_offsets, size_t n,
                                   size_t jpg_bytes, uint32_t width, uint32_t height, const ucfp_image_preprocess* pre,
                                   const uint8_t* d_exact, uint8_t* d_out, int32_t* d_status, void* stream);

/* Micro-batcher for JPEG uploads: the object of ucfp_png_batcher_create with the JPEG front end behind it (records of the
 * files' luma planes).  Submit / stats / destroy with the ucfp_png_batcher_* calls. */
int ucfp_jpeg_batcher_create(ucfp_ctx* ctx, uint32_t algo, uint32_t width, uint32_t height, const ucfp_image_preprocess* pre,
                             size_t max_batch, size_t max_bytes, uint32_t max_delay_us, ucfp_png_batcher** out);

/* BLAKE3-256 (default hash mode) of a HOST buffer: the `exact` digest the reference stores in
 * ImageFingerprint.exact (BLAKE3 of the uploaded bytes). Host code; no device needed. */
int ucfp_blake3(const uint8_t* data, size_t len, uint8_t out[32]);

/* =============================== STORED TABLES ====================
 * The reference's source of truth is one redb file: tables ucfp/fingerprints/v1, ucfp/vectors/v1, ucfp/catalog/v2,
 * all keyed (tenant_id, record_id) and written in one transaction per upsert (src/index/embedded/mod.rs:37-43,
 * :157-227); EmbeddedBackend::open (:104-125) is where a device mirror has to be rebuilt.  redb's page format lives in
 * a crate outside the tree, so the drop-in keeps a SIDECAR: an append-only log of exactly those rows (fingerprint
 * bytes, embedding, the catalog row's serde_json text) that the host appends to right after its redb transaction
 * commits, and replays at start-up.  Last entry of a key wins; a torn tail is cut on the next open (CRC per entry).
 * Host-only calls (no GPU involved). */
typedef struct ucfp_sidecar ucfp_sidecar;
int ucfp_sidecar_open(const char* path, ucfp_sidecar** out);      /* creates the log if missing, validates it otherwise */
void ucfp_sidecar_close(ucfp_sidecar* sc);
/* One call per record of IndexBackend::upsert (mod.rs:176-208): embedding NULL / dim 0 = "no vector" (:184-191). */
int ucfp_sidecar_append_upsert(ucfp_sidecar* sc, uint32_t tenant, uint64_t record_id, const uint8_t* fingerprint,
                               uint32_t fp_len, const float* embedding, uint32_t dim, const char* catalog_json,
                               uint32_t json_len);
int ucfp_sidecar_append_delete(ucfp_sidecar* sc, uint32_t tenant, uint64_t record_id);   /* IndexBackend::delete :229-266 */
int ucfp_sidecar_sync(ucfp_sidecar* sc);                           /* fdatasync: call where the host fsyncs redb */

/* Read side: the live rows of a log (after replaying overwrites and deletes), in ascending (tenant, record_id) order
 * -- the order of the reference's range scans.  Pointers returned by _row point into the mapped file and live until
 * _close; embedding bytes are not necessarily 4-byte aligned. */
typedef struct ucfp_sidecar_snapshot ucfp_sidecar_snapshot;
int ucfp_sidecar_snapshot_open(const char* path, ucfp_sidecar_snapshot** out, uint64_t* live_rows, uint64_t* log_entries,
                               uint64_t* torn_bytes);
void ucfp_sidecar_snapshot_close(ucfp_sidecar_snapshot* s);
int ucfp_sidecar_snapshot_row(ucfp_sidecar_snapshot* s, uint64_t i, uint32_t* tenant, uint64_t* record_id,
                              const uint8_t** fingerprint, uint32_t* fp_len, const uint8_t** embedding_bytes, uint32_t* dim,
                              const char** catalog_json, uint32_t* json_len);
/* Bulk gathers for the rebuild: fingerprints of the rows whose catalog `algorithm` is `algorithm` and whose blob is
 * fp_len bytes ("only comparable hashes share an index"), or the embeddings of one dimension, packed into caller arrays
 * (any of which may be NULL).  *n = matching rows; if it exceeds cap only the first cap were written. */
int ucfp_sidecar_snapshot_gather_fingerprints(ucfp_sidecar_snapshot* s, const char* algorithm, uint32_t fp_len,
                                              uint32_t* tenants, uint64_t* ids, uint8_t* fingerprints, uint64_t cap,
                                              uint64_t* n);
int ucfp_sidecar_snapshot_gather_vectors(ucfp_sidecar_snapshot* s, uint32_t dim, uint32_t* tenants, uint64_t* ids,
                                         float* rows, uint64_t cap, uint64_t* n);

#ifdef __cplusplus
}
#endif
#endif /* UCFP_HIP_H */
