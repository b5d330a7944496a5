// text_core.h -- what the text hashing kernels share (text.hip: whole documents; text_streams.hip: streams): the LDS
// batch of one wave and its limits, the ASCII word rule, XXH3 read from LDS, the MinHash second hash.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ucfp_hip.h"
#include "../../include/ucfp_xxh3.h"
#include "common.h"

namespace ucfp {

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kTokCap = 256;        // tokens per LDS batch
constexpr int kCanonCap = 1536;     // canonical bytes per LDS batch
constexpr int kStepTok = 33;        // a 64-byte step can open at most 32 (+1 carried) tokens
constexpr int kStepRoom = 130;      // canonical bytes a step may add (64 + 32 separators), with margin
// what survives a flush is a prefix of one k-token window: it must leave room for the next step (derivation in ucfp_hip.h)
static_assert(kCanonCap - kStepRoom - 1 == UCFP_TEXT_MAX_WINDOW_BYTES, "the documented -2 limit follows these constants");

struct WaveLds {
    uint8_t stage[256 + 8];
    uint8_t canon[kCanonCap + 72];
    uint16_t cstart[kTokCap + 8];
    uint16_t cend[kTokCap + 8];
    uint64_t h1[kTokCap];
    uint64_t h2[kTokCap];
};

enum { C_O = 0, C_L = 1, C_N = 2, C_ML = 3, C_MNL = 4, C_MN = 5 };

__device__ __forceinline__ int cls(uint32_t c) {
    const uint32_t lc = c | 0x20u;
    int r = C_O;
    r = (lc - 'a' <= 25u || c == '_') ? C_L : r;
    r = (c - '0' <= 9u) ? C_N : r;
    r = (c == ':') ? C_ML : r;
    r = (c == '.' || c == '\'') ? C_MNL : r;
    r = (c == ',' || c == ';') ? C_MN : r;
    return r;
}

__device__ __forceinline__ bool inword(uint32_t p, uint32_t c, uint32_t q, bool pretok) {
    if (pretok) return c != ' ';   // every other byte, 0x00 included (the caller's `pos < len` guards the padding)
    const int cc = cls(c), pc = cls(p), qc = cls(q);
    const bool mid_l = (cc == C_ML || cc == C_MNL) && pc == C_L && qc == C_L;   // WB6/7
    const bool mid_n = (cc == C_MN || cc == C_MNL) && pc == C_N && qc == C_N;   // WB11/12
    return cc == C_L || cc == C_N || mid_l || mid_n;
}

// XXH3 over the canonical token stream in LDS.  Unaligned 8 / 4-byte words come from ALIGNED dwords and
// v_alignbyte (3 + 2 or 2 + 1 instructions instead of 8 / 4 byte loads and a shift/or ladder); the stream has
// 72 bytes of slack behind it, so the dword past the end is readable.  The hash body is force-inlined, which
// also keeps the pointer in the LDS address space (ds_read, not flat loads).
#define UCFP_RD8_LDS(p, i) ((p)[(i)])
__device__ __forceinline__ uint64_t xxh3_lds_rd64(const uint8_t* src, size_t o) {
    const uint8_t* q = src + o;
    const uint32_t sh = (uint32_t)reinterpret_cast<uintptr_t>(q) & 3u;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(q - sh);   // pointer arithmetic keeps the LDS address space
    const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
    return (uint64_t)__builtin_amdgcn_alignbyte(d1, d0, sh) | ((uint64_t)__builtin_amdgcn_alignbyte(d2, d1, sh) << 32);
}
__device__ __forceinline__ uint32_t xxh3_lds_rd32(const uint8_t* src, size_t o) {
    const uint8_t* q = src + o;
    const uint32_t sh = (uint32_t)reinterpret_cast<uintptr_t>(q) & 3u;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(q - sh);
    return __builtin_amdgcn_alignbyte(p[1], p[0], sh);
}
UCFP_XXH3_DEFINE_BODY(xxh3_lds, const uint8_t*, UCFP_RD8_LDS)

__device__ __forceinline__ uint64_t mix_h2(uint64_t h1) {
    uint64_t z = h1 + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (z ^ (z >> 31)) | 1ull;
}

__device__ __forceinline__ uint32_t popc_below(uint64_t m, int lane) {  // bits of m below `lane`
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    (void)lane;
}

__device__ __forceinline__ void wave_sync() { wave_lds_sync(); }
}  // namespace

}  // namespace ucfp
