// multi_plan.h -- the host planner of the multi-tenant Hamming search (DESIGN M3; hamming_multi.hip, index.hip).
//
// A batch in which every query names its own tenant becomes, on the host:
//   perm      the query numbers sorted by tenant, stable (position p of the sorted batch is query perm[p])
//   pos_seg   the segment of every position
//   segs      one per distinct tenant: the shard's rows / ids / n and its run [first, first + count) of positions
//   items     the work of one workgroup each: rows [tile kTileRows, (tile + 1) kTileRows) of a segment against positions
//             [first + q0, first + q0 + nq) of it, nq <= kQueryChunk.  Tiles vary slowest inside a segment, so the workgroups
//             that share a tile of rows are neighbours.
// Every (query, row) pair of the batch lies in exactly one item; a segment without rows has none.
// Plain C++ (no HIP): tests/native/multi_plan_check.cpp drives it without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ucfp {
namespace multi {

constexpr uint32_t kBlock = 256;         // threads of a histogram / collect workgroup
constexpr uint32_t kTileRows = 1024;     // rows of an item: four coalesced u64 loads per lane
constexpr uint32_t kQueryChunk = 16;     // queries of an item: its LDS histogram is [16][65] words
constexpr uint32_t kTieCap = 512;        // ids of a query's tie list; more ties at tau take the gated exact pass
constexpr uint32_t kMaxBatch = 16384;    // positions of one plan: a larger batch is planned and run in chunks of this
constexpr uint64_t kMaxItems = 0xffffffffull / kBlock;   // grid x block has to fit 32 bits
constexpr uint64_t kMaxRows = 0xffffffffull;             // the histograms count rows in 32 bits

enum { kPlanOk = 0, kPlanTooManyItems = 1, kPlanTooManyRows = 2 };

struct ShardRef {        // what the planner needs of a tenant's shard (n = 0: unknown tenant or no rows)
    const uint64_t* rows = nullptr;
    const uint64_t* ids = nullptr;
    uint64_t n = 0;
};

struct Seg {             // device image: 32 bytes
    const uint64_t* rows;
    const uint64_t* ids;
    uint64_t n;
    uint32_t first, count;
};

struct Item {            // device image: 16 bytes
    uint32_t seg, tile, q0, nq;
};

struct Plan {
    std::vector<uint32_t> perm, pos_seg;
    std::vector<Seg> segs;
    std::vector<uint32_t> seg_tenant;    // host only
    std::vector<Item> items;
    uint64_t item_count = 0;             // set even when the plan is refused
};

inline uint64_t seg_items(uint64_t n, uint32_t count) {
    const uint64_t tiles = n / kTileRows + (n % kTileRows ? 1 : 0);
    const uint64_t chunks = ((uint64_t)count + kQueryChunk - 1) / kQueryChunk;
    if (tiles > kMaxItems) return tiles;     // refused whatever the chunks: no product that could wrap
    return tiles * chunks;                   // (< 2^24 x 2^29)
}

// lookup(tenant) -> ShardRef.  nq <= 2^32 - 1.  A refused plan holds no items.
template <class Lookup>
int plan(const uint32_t* tenants, size_t nq, Lookup&& lookup, Plan* out) {
    out->perm.clear();
    out->pos_seg.clear();
    out->segs.clear();
    out->seg_tenant.clear();
    out->items.clear();
    out->item_count = 0;
    if (nq == 0) return kPlanOk;
    std::vector<uint64_t> key(nq);    // (tenant, query number): sorting the keys is the stable sort by tenant
    for (size_t i = 0; i < nq; i++) key[i] = ((uint64_t)tenants[i] << 32) | (uint64_t)i;
    std::sort(key.begin(), key.end());
    out->perm.resize(nq);
    out->pos_seg.resize(nq);
    for (size_t p = 0; p < nq; p++) {
        const uint32_t t = (uint32_t)(key[p] >> 32);
        out->perm[p] = (uint32_t)key[p];
        if (p == 0 || t != out->seg_tenant.back()) {
            const ShardRef s = lookup(t);
            Seg g;
            g.rows = s.n ? s.rows : nullptr;
            g.ids = s.n ? s.ids : nullptr;
            g.n = s.n;
            g.first = (uint32_t)p;
            g.count = 0;
            out->segs.push_back(g);
            out->seg_tenant.push_back(t);
        }
        out->segs.back().count++;
        out->pos_seg[p] = (uint32_t)(out->segs.size() - 1);
    }
    uint64_t total = 0;
    bool rows_over = false;
    for (const Seg& g : out->segs) {
        const uint64_t it = seg_items(g.n, g.count);
        total = total + it < total ? ~0ull : total + it;
        rows_over = rows_over || g.n > kMaxRows;
    }
    out->item_count = total;
    if (total > kMaxItems) return kPlanTooManyItems;
    if (rows_over) return kPlanTooManyRows;
    out->items.reserve((size_t)total);
    for (size_t s = 0; s < out->segs.size(); s++) {
        const Seg& g = out->segs[s];
        const uint32_t tiles = (uint32_t)(g.n / kTileRows + (g.n % kTileRows ? 1 : 0));
        for (uint32_t t = 0; t < tiles; t++)
            for (uint32_t q0 = 0; q0 < g.count; q0 += kQueryChunk) {
                Item it;
                it.seg = (uint32_t)s;
                it.tile = t;
                it.q0 = q0;
                it.nq = g.count - q0 < kQueryChunk ? g.count - q0 : kQueryChunk;
                out->items.push_back(it);
            }
    }
    return kPlanOk;
}

}  // namespace multi
}  // namespace ucfp
