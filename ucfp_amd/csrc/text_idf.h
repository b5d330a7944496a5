// text_idf.h -- what the tokeniser kernels and text_idf.hip share for TF.IDF SimHash: the arguments of the
// two extra modes of text_flush (text_core.h) and the launchers of the four token sources in those modes.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct ucfp_ctx;
struct ucfp_idf_table;

namespace ucfp {

// T_IDF reads the table; T_KEYS writes keys and ordinals; T_MIN and T_SIM never touch it.
struct TextIdfAux {
    // T_IDF: the table, open addressing with linear probing.  Slot i holds the key tab_keys[i] != 0 or is empty (0); key 0
    // itself lives in the extra slot `cap` = mask + 1, whose weight is the default while the key is absent.  The table is
    // at most half full (text_idf.hip, kIdfLoadDen), so the probe of an absent key ends at an empty slot.
    const uint64_t* tab_keys = nullptr;
    const uint32_t* tab_wts = nullptr;
    uint32_t shift = 63;      // home slot = (key * kIdfMul) >> shift
    uint32_t mask = 1;        // capacity - 1
    uint32_t default_w = 0;
    // T_KEYS: token t of a document goes to slot slot0 + t, t < doc_cap (a document has no more tokens than bytes)
    uint32_t doc_cap = 0;     // (set per wave)
    uint64_t* key_out = nullptr;
    uint32_t* ord_out = nullptr;
    uint64_t slot_base = 0;   // byte offset of the piece's first document: a document's slots begin at its own byte offset
    uint64_t slot_cap = 0;    // slots of the piece
    uint64_t slot0 = 0;       // (set per wave)
    uint32_t ord = 0;         // (set per wave) the document's ordinal in the piece
};
constexpr uint64_t kIdfMul = 0x9E3779B97F4A7C15ull;

// text_idf.hip: the T_IDF arguments of a table as it stands now (a kernel launched with them must not outlive a change of
// the table); *is_final: its weights are set (T9.6), *device: where it lives.  Either pointer may be NULL.  A stream set
// (text_streams.hip) calls this at every push.
TextIdfAux idf_table_aux(const ucfp_idf_table* t, bool* is_final, int* device);

// text.hip: the word tokeniser (modes RAW_ASCII and PRETOKENIZED); idf = true the weighted record, false the keys
int launch_text_idf_words(bool idf, const TextIdfAux& aux, const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode,
                          uint8_t* out, int32_t* status, hipStream_t stream);
// text_grapheme.hip: src 0 = ASCII graphemes, 1 = graphemes of a canonical stream, 2 = the caller's token table (`offsets` =
// doc_tokens, tok_off its byte offsets)
int launch_text_idf_marked(int src, bool idf, const TextIdfAux& aux, const uint8_t* bytes, const uint64_t* offsets,
                           const uint64_t* tok_off, size_t n, uint8_t* out, int32_t* status, hipStream_t stream);
// text_grapheme.hip: the grapheme canon pass on its own (count, scan, emit): can_off n + 1 words, cstatus n words
int launch_text_gcanon(ucfp_ctx* ctx, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, uint8_t* canon, uint64_t* can_off,
                       int32_t* cstatus, hipStream_t stream);

}  // namespace ucfp
