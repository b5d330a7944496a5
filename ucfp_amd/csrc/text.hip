// text.hip -- batched MinHash-128 and SimHash-64 for gfx950.
//
// Replaces the arithmetic behind text::fingerprint_minhash_with::<128> (src/modality/text.rs:182-236)
// and simhash_dispatch (text.rs:366-421) of the reference, i.e. txtfp's MinHashFingerprinter /
// SimHashFingerprinter, for documents that are ASCII (canonicalisation = lower-casing, UAX#29 word
// segmentation restricted to ASCII, both done here on the GPU) or that the host has already
// canonicalised and tokenised (PRETOKENIZED: tokens separated by single spaces).  Spec: DESIGN.md
// "Text spec" T1..T6; CPU statement: oracle/ (text).
//
// ONE WAVE PER DOCUMENT, no workgroup barrier anywhere.  The wave is the tokenizer:
//   A  64 bytes per step, lane = byte.  "Byte is inside a word" is a function of (prev, cur, next)
//      only (WB5-13 on ASCII), so one __ballot gives the 64-bit word mask of the step; token starts,
//      token ends, a byte's rank among word bytes and its token index are shifts, ANDs and
//      popcounts (v_mbcnt) of that mask -- no scan, no LDS traffic besides the output itself.
//   B  every word byte is written (lower-cased) to its place in the CANONICAL STREAM
//      tok0 ' ' tok1 ' ' ...  in LDS; a k-shingle is one contiguous byte range of that stream.
//   C  when the LDS batch fills (256 tokens / 1.5 KiB) or the document ends: lane = shingle (MinHash)
//      or token (SimHash) hashes its byte range with XXH3_64 straight from LDS,
//   D  then lane = 2 of the 128 slots: every shingle's (h1, h2) is broadcast from LDS and each lane
//      keeps running minima of h1 + i*h2 for its slots i and i + 64 (a wave = all 128 permutations);
//      SimHash: lane = output bit, each token hash is broadcast and lane b counts bit b.
//      The last k-1 complete tokens (and an unfinished one) are carried to the front of the batch.
//      MinHash with H slots: lane = ceil(H / 64) of the H slots, i, i + 64, i + 128, ...
// ALU-bound: ~16 integer ops per shingle per lane in D; HBM traffic is 4 KiB + 1 KiB per document.
//
// A, B (text_step), C, D (text_flush) and the record (text_emit) live in text_core.h, which text_stream_kernel
// (text_streams.hip) calls as well: the kernel below is the document's byte reader around them.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "text_core.h"

namespace ucfp {

// MODE = T_MIN (false): MinHash (out 1032 B/doc); T_SIM (true): SimHash (out 8 B/doc); T_IDF: weighted SimHash against the
// table in `aux` (out 8 B/doc); T_KEYS: no record, the tokens' keys go to aux.key_out (text_core.h).  NR = 0: the 128-slot
// record, `h` unused; NR >= 1 (T_MIN only): h slots, 64 (NR - 1) < h <= 64 NR, out 8 + 8 h B/doc.
template <int MODE, int NR = 0>
__global__ __launch_bounds__(64 * kWavesPerBlock) void text_hash_kernel(
    const uint8_t* __restrict__ utf8, const uint64_t* __restrict__ offsets, size_t n, int pretok_i, uint32_t k,
    uint8_t* __restrict__ out, int32_t* __restrict__ status, TextIdfAux aux, uint32_t h) {
    constexpr int R = NR ? NR : 2;
    const uint32_t slots = NR ? h : 128u;
    __shared__ WaveLds lds[kWavesPerBlock];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t doc = (size_t)blockIdx.x * kWavesPerBlock + wave;
    if (doc >= n) return;  // whole wave
    WaveLds& L = lds[wave];
    const bool pretok = pretok_i != 0;
    const uint8_t* __restrict__ text = utf8 + offsets[doc];
    const size_t len = (size_t)(offsets[doc + 1] - offsets[doc]);
    const bool aligned4 = (reinterpret_cast<uintptr_t>(text) & 3u) == 0;

    TextWave W;
    uint64_t mx[text_mx_len(R)];
#pragma unroll
    for (int r = 0; r < text_mx_len(R); r++) mx[r] = ~0ull;
    bool nonascii = false, too_long = false;
    if (MODE == T_KEYS) text_keys_doc(aux, offsets[doc], len, doc);

    // ---- stream the document, 256 bytes per outer iteration, 64 per step ----
    auto load_chunk = [&](size_t base) -> uint32_t {  // this lane's 4 bytes of [base, base + 256)
        const size_t o = base + 4 * (size_t)lane;
        if (o >= len) return 0u;
        if (aligned4 && o + 4 <= len) return *reinterpret_cast<const uint32_t*>(text + o);
        uint32_t v = 0;
        for (int j = 0; j < 4; j++)
            if (o + j < len) v |= (uint32_t)text[o + j] << (8 * j);
        return v;
    };
    uint32_t cur = load_chunk(0);
    for (size_t base = 0; base < len && !too_long; base += 256) {
        const uint32_t nxt = load_chunk(base + 256);
        wave_sync();
        *reinterpret_cast<uint32_t*>(&L.stage[4 * lane]) = cur;
        if (lane == 0) *reinterpret_cast<uint32_t*>(&L.stage[256]) = __builtin_amdgcn_readfirstlane(nxt);
        wave_sync();
        if (!pretok) nonascii |= (cur & 0x80808080u) != 0;
#pragma unroll 1
        for (int sub = 0; sub < 4; sub++) {
            const size_t pos = base + 64 * sub + lane;
            if (base + 64 * sub >= len) break;
            if (text_batch_full(W)) {   // make room
                text_flush<MODE, R>(L, W, k, lane, false, &aux, mx);
                if (text_batch_full(W)) too_long = true;
                if (too_long) break;
            }
            (void)text_step(L, W, sub, pos, len, pretok, lane);
        }
        cur = nxt;
    }
    // close a token that runs to the end of the document, then the final flush
    if (W.carry && W.ntok > 0 && lane == 0) L.cend[W.ntok - 1] = (uint16_t)(W.cbase + W.ntok - 1);
    if (!too_long) text_flush<MODE, R>(L, W, k, lane, true, &aux, mx);
    // ---- emit ----
    const int32_t stv = text_emit<MODE, R>(out + doc * (MODE != T_MIN ? 8 : 8 + 8 * (size_t)slots), W, __ballot(nonascii) != 0,
                                           too_long, lane, slots, mx);
    if (status && lane == 0) status[doc] = stv;
}

namespace {
template <int NR>
void launch_minhash_nr(const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode, uint32_t k, uint32_t h, uint8_t* out,
                       int32_t* status, hipStream_t stream) {
    const unsigned grid = (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL((text_hash_kernel<T_MIN, NR>), dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, utf8, offsets, n, mode, k,
                       out, status, TextIdfAux{}, h);
}
}  // namespace

// h = 128 is the kernel this call has always launched; any other h (validated by the caller, minhash_h_check) goes to
// the instantiation of text_minhash_nr(h) minima per lane
int launch_text_minhash(const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode, uint32_t k,
                        uint8_t* out, int32_t* status, hipStream_t stream, uint32_t h) {
    if (n == 0) return 0;
    if (h == 128) {
        launch_minhash_nr<0>(utf8, offsets, n, mode, k, h, out, status, stream);
        return 0;
    }
    switch (text_minhash_nr(h)) {
        case 1: launch_minhash_nr<1>(utf8, offsets, n, mode, k, h, out, status, stream); break;
        case 2: launch_minhash_nr<2>(utf8, offsets, n, mode, k, h, out, status, stream); break;
        case 3: launch_minhash_nr<3>(utf8, offsets, n, mode, k, h, out, status, stream); break;
        case 4: launch_minhash_nr<4>(utf8, offsets, n, mode, k, h, out, status, stream); break;
        case 6: launch_minhash_nr<6>(utf8, offsets, n, mode, k, h, out, status, stream); break;
        case 8: launch_minhash_nr<8>(utf8, offsets, n, mode, k, h, out, status, stream); break;
        case 12: launch_minhash_nr<12>(utf8, offsets, n, mode, k, h, out, status, stream); break;
        default: launch_minhash_nr<16>(utf8, offsets, n, mode, k, h, out, status, stream); break;
    }
    return 0;
}

int launch_text_simhash(const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode, uint8_t* out,
                        int32_t* status, hipStream_t stream) {
    if (n == 0) return 0;
    const unsigned grid = (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(text_hash_kernel<T_SIM>, dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, utf8, offsets, n,
                       mode, 1u, out, status, TextIdfAux{}, 0u);
    return 0;
}

// the word tokeniser in the two modes of DESIGN.md T9 (text_idf.hip): idf = true the weighted record, false the keys
int launch_text_idf_words(bool idf, const TextIdfAux& aux, const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode,
                          uint8_t* out, int32_t* status, hipStream_t stream) {
    if (n == 0) return 0;
    const unsigned grid = (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock);
    if (idf)
        hipLaunchKernelGGL(text_hash_kernel<T_IDF>, dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, utf8, offsets, n, mode, 1u,
                           out, status, aux, 0u);
    else
        hipLaunchKernelGGL(text_hash_kernel<T_KEYS>, dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, utf8, offsets, n, mode, 1u,
                           out, status, aux, 0u);
    return 0;
}

}  // namespace ucfp
