// roaring_parse.h -- parser of a query filter: the portable serialization of a 64-bit Roaring treemap (DESIGN F1, F2).
//
// Plain C++ without HIP, so that it also compiles on its own (tests/native/roaring_parse_check.cpp runs it under the
// host sanitizers).  parse() validates the bytes and, when asked, flattens both levels of the treemap into one sorted
// directory -- key = id >> 16 -- over a repacked payload image in which arrays are 2-byte aligned, run pairs 4-byte
// aligned and bitmaps 8-byte aligned (serialized containers are not even 2-byte aligned behind an odd run-flag bitset).
// The device probe (index_filter.hip) reads only that image.  Nothing outside [bytes, bytes + len) is ever read.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace ucfp {
namespace roaring {

constexpr uint64_t kMaxBytes = 0xFFFFFFFFull;        // a filter of up to 2^32 - 1 bytes ...
constexpr uint64_t kMaxContainers = 1ull << 24;      // ... and up to 2^24 containers over all its 32-bit bitmaps
constexpr uint32_t kArray = 0, kBitmap = 1, kRun = 2;

struct Entry {          // one container of the flat directory (16 bytes, read by the device as two 8-byte words)
    uint64_t off;       // byte offset of its payload in the image
    uint32_t n;         // array: values; run: pairs; bitmap: 1024
    uint32_t type;      // kArray / kBitmap / kRun
};

struct Parsed {
    std::vector<uint64_t> keys;      // id >> 16 of every container, strictly ascending
    std::vector<Entry> ents;
    std::vector<uint8_t> image;      // arrays: u16 values; runs: u32 = start | (length - 1) << 16; bitmaps: 1024 x u64
};

namespace detail {

struct Reader {
    const uint8_t* b;
    size_t len, pos = 0;
    char* err;
    size_t errlen;
    bool need(size_t k, const char* what) {
        if (len - pos >= k) return true;
        fail(pos, what);
        return false;
    }
    void fail(size_t at, const char* what) {
        if (err && errlen) snprintf(err, errlen, "roaring filter: %s at byte %zu", what, at);
    }
    uint16_t u16(size_t at) const { return (uint16_t)(b[at] | (uint16_t)b[at + 1] << 8); }
    uint32_t u32(size_t at) const { return (uint32_t)u16(at) | (uint32_t)u16(at + 2) << 16; }
    uint64_t u64(size_t at) const { return (uint64_t)u32(at) | (uint64_t)u32(at + 4) << 32; }
};

inline void image_align(std::vector<uint8_t>& img, size_t a) { img.resize((img.size() + a - 1) / a * a, 0); }
inline void image_put16(std::vector<uint8_t>& img, uint16_t v) {
    img.push_back((uint8_t)v);
    img.push_back((uint8_t)(v >> 8));
}

}  // namespace detail

// 0 = valid.  `out` (may be NULL: validate only) receives the directory and the image; `cardinality` (may be NULL) the number
// of ids in the set; `err` a message that names the byte offset of the first fault.
inline int parse(const uint8_t* bytes, size_t len, Parsed* out, uint64_t* cardinality, char* err, size_t errlen) {
    using namespace detail;
    if (cardinality) *cardinality = 0;
    if (out) {
        out->keys.clear();
        out->ents.clear();
        out->image.clear();
    }
    Reader r{bytes, len, 0, err, errlen};
    if (!bytes && len) {
        r.fail(0, "bytes is NULL");
        return -1;
    }
    if ((uint64_t)len > kMaxBytes) {
        r.fail(0, "filter larger than 2^32 - 1 bytes");
        return -1;
    }
    if (!r.need(8, "truncated treemap count")) return -1;
    const uint64_t nmaps = r.u64(0);
    r.pos = 8;
    if (nmaps > (1ull << 32)) {
        r.fail(0, "treemap count above 2^32");
        return -1;
    }
    uint64_t card_total = 0, containers = 0;
    int64_t prev_high = -1;
    for (uint64_t m = 0; m < nmaps; m++) {
        if (!r.need(4, "truncated high key")) return -1;
        const uint32_t high = r.u32(r.pos);
        if ((int64_t)high <= prev_high) {
            r.fail(r.pos, "high keys not strictly ascending");
            return -1;
        }
        prev_high = high;
        r.pos += 4;
        const size_t base = r.pos;      // offsets of the offset header count from here
        if (!r.need(4, "truncated cookie")) return -1;
        const uint32_t cookie = r.u32(r.pos);
        uint32_t n = 0;
        size_t flags_at = 0;
        bool has_runs = false;
        if (cookie == 12346u) {
            if (!r.need(8, "truncated container count")) return -1;
            n = r.u32(r.pos + 4);
            if (n > 65536u) {
                r.fail(r.pos + 4, "more than 65536 containers in a 32-bit bitmap");
                return -1;
            }
            r.pos += 8;
        } else if ((cookie & 0xFFFFu) == 12347u) {
            has_runs = true;
            n = (cookie >> 16) + 1;
            r.pos += 4;
            if (!r.need((n + 7) / 8, "truncated run-flag bitset")) return -1;
            flags_at = r.pos;
            r.pos += (n + 7) / 8;
        } else {
            r.fail(r.pos, "unknown cookie");
            return -1;
        }
        containers += n;
        if (containers > kMaxContainers) {
            r.fail(base, "more than 2^24 containers");
            return -1;
        }
        if (!r.need((size_t)n * 4, "truncated descriptive header")) return -1;
        const size_t desc_at = r.pos;
        r.pos += (size_t)n * 4;
        int32_t prev_key = -1;
        for (uint32_t i = 0; i < n; i++) {
            const uint16_t key = r.u16(desc_at + (size_t)i * 4);
            if ((int32_t)key <= prev_key) {
                r.fail(desc_at + (size_t)i * 4, "container keys not strictly ascending");
                return -1;
            }
            prev_key = key;
        }
        const bool has_offsets = !has_runs || n >= 4;
        const size_t offs_at = r.pos;
        if (has_offsets) {
            if (!r.need((size_t)n * 4, "truncated offset header")) return -1;
            r.pos += (size_t)n * 4;
        }
        for (uint32_t i = 0; i < n; i++) {
            const uint16_t key = r.u16(desc_at + (size_t)i * 4);
            const uint32_t card = (uint32_t)r.u16(desc_at + (size_t)i * 4 + 2) + 1;
            const bool is_run = has_runs && ((bytes[flags_at + i / 8] >> (i % 8)) & 1u);
            if (has_offsets && (uint64_t)r.u32(offs_at + (size_t)i * 4) != (uint64_t)(r.pos - base)) {
                r.fail(offs_at + (size_t)i * 4, "offset header entry differs from where the container lies");
                return -1;
            }
            Entry e{0, 0, 0};
            if (is_run) {
                if (!r.need(2, "truncated run count")) return -1;
                const uint32_t nruns = r.u16(r.pos);
                if (!r.need(2 + (size_t)nruns * 4, "truncated run container")) return -1;
                const size_t at = r.pos + 2;
                int32_t prev_end = -1;
                uint32_t total = 0;
                for (uint32_t j = 0; j < nruns; j++) {
                    const uint32_t start = r.u16(at + (size_t)j * 4), lm1 = r.u16(at + (size_t)j * 4 + 2);
                    if ((int32_t)start <= prev_end) {
                        r.fail(at + (size_t)j * 4, "runs unsorted or overlapping");
                        return -1;
                    }
                    if (start + lm1 > 65535u) {
                        r.fail(at + (size_t)j * 4, "run passes 65535");
                        return -1;
                    }
                    prev_end = (int32_t)(start + lm1);
                    total += lm1 + 1;
                }
                if (total != card) {
                    r.fail(r.pos, "run container total differs from its header cardinality");
                    return -1;
                }
                if (out) {
                    image_align(out->image, 4);
                    e = Entry{out->image.size(), nruns, kRun};
                    for (uint32_t j = 0; j < nruns; j++) {
                        image_put16(out->image, r.u16(at + (size_t)j * 4));
                        image_put16(out->image, r.u16(at + (size_t)j * 4 + 2));
                    }
                }
                r.pos = at + (size_t)nruns * 4;
            } else if (card <= 4096u) {
                if (!r.need((size_t)card * 2, "truncated array container")) return -1;
                int32_t prev = -1;
                for (uint32_t j = 0; j < card; j++) {
                    const uint16_t v = r.u16(r.pos + (size_t)j * 2);
                    if ((int32_t)v <= prev) {
                        r.fail(r.pos + (size_t)j * 2, "array not strictly ascending");
                        return -1;
                    }
                    prev = v;
                }
                if (out) {
                    image_align(out->image, 2);
                    e = Entry{out->image.size(), card, kArray};
                    out->image.insert(out->image.end(), bytes + r.pos, bytes + r.pos + (size_t)card * 2);
                }
                r.pos += (size_t)card * 2;
            } else {
                if (!r.need(8192, "truncated bitmap container")) return -1;
                uint32_t pop = 0;
                for (uint32_t j = 0; j < 1024; j++) pop += (uint32_t)__builtin_popcountll(r.u64(r.pos + (size_t)j * 8));
                if (pop != card) {      // (card > 4096 here, so a population <= 4096 is refused too)
                    r.fail(r.pos, "bitmap population differs from its header cardinality");
                    return -1;
                }
                if (out) {
                    image_align(out->image, 8);
                    e = Entry{out->image.size(), 1024u, kBitmap};
                    out->image.insert(out->image.end(), bytes + r.pos, bytes + r.pos + 8192);
                }
                r.pos += 8192;
            }
            card_total += card;
            if (out) {
                out->keys.push_back((uint64_t)high << 16 | key);
                out->ents.push_back(e);
            }
        }
    }
    if (r.pos != len) {
        r.fail(r.pos, "trailing bytes");
        return -1;
    }
    if (cardinality) *cardinality = card_total;
    return 0;
}

// Membership of `id` in a parsed filter: the host statement of what the device probe computes.
inline bool contains(const Parsed& p, uint64_t id) {
    const uint64_t key = id >> 16;
    const uint32_t low = (uint32_t)(id & 0xFFFFu);
    size_t lo = 0, hi = p.keys.size();
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (p.keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    if (lo == p.keys.size() || p.keys[lo] != key) return false;
    const Entry& e = p.ents[lo];
    const uint8_t* c = p.image.data() + e.off;
    if (e.type == kBitmap) return (c[low >> 3] >> (low & 7u)) & 1u;
    size_t a = 0, b = e.n;
    if (e.type == kArray) {
        while (a < b) {
            const size_t mid = (a + b) / 2;
            const uint32_t v = (uint32_t)(c[mid * 2] | c[mid * 2 + 1] << 8);
            if (v < low) a = mid + 1;
            else b = mid;
        }
        return a < e.n && (uint32_t)(c[a * 2] | c[a * 2 + 1] << 8) == low;
    }
    while (a < b) {      // the last run that starts at or below `low`
        const size_t mid = (a + b) / 2;
        if ((uint32_t)(c[mid * 4] | c[mid * 4 + 1] << 8) <= low) a = mid + 1;
        else b = mid;
    }
    if (a == 0) return false;
    const uint8_t* pr = c + (a - 1) * 4;
    return low - (uint32_t)(pr[0] | pr[1] << 8) <= (uint32_t)(pr[2] | pr[3] << 8);
}

}  // namespace roaring
}  // namespace ucfp
