// multi_plan_check.cpp -- the planner of the multi-tenant search (ucfp_amd/csrc/multi_plan.h) against a naive model.
// Stand-alone host program (tests/test_multi_plan.py builds it with -fsanitize=address,undefined): prints "ok ..." and exits 0.
//
// For every scenario: perm is a permutation; the segments partition it by tenant, tenants ascending, query numbers ascending
// inside a segment (the stable order); every segment carries what the lookup gave for its tenant; every (query, row) pair
// is covered by exactly one item, no item is empty or reaches past its segment; item_count is the number of items.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "../../ucfp_amd/csrc/multi_plan.h"

namespace m = ucfp::multi;

static int g_checks = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        g_checks++;                                                           \
        if (!(c)) {                                                           \
            printf("FAILED %s:%d: %s  [scenario %s]\n", __FILE__, __LINE__, #c, g_name); \
            exit(1);                                                          \
        }                                                                     \
    } while (0)
static const char* g_name = "";

// rows / ids pointers are never followed: distinct fake addresses per tenant
static m::ShardRef fake(uint32_t tenant, uint64_t n) {
    m::ShardRef r;
    r.rows = reinterpret_cast<const uint64_t*>((uintptr_t)0x100000 + (uintptr_t)tenant * 16);
    r.ids = reinterpret_cast<const uint64_t*>((uintptr_t)0x100008 + (uintptr_t)tenant * 16);
    r.n = n;
    return r;
}

static void run(const char* name, const std::vector<uint32_t>& tenants, const std::map<uint32_t, uint64_t>& sizes, int expect,
                bool count_pairs = true) {
    g_name = name;
    m::Plan p;
    auto lookup = [&](uint32_t t) {
        auto it = sizes.find(t);
        return it == sizes.end() ? m::ShardRef() : fake(t, it->second);
    };
    const int rc = m::plan(tenants.data(), tenants.size(), lookup, &p);
    CHECK(rc == expect);
    const size_t nq = tenants.size();
    // naive item count
    std::map<uint32_t, uint32_t> per_tenant;
    for (uint32_t t : tenants) per_tenant[t]++;
    unsigned __int128 want_items = 0;
    for (auto& kv : per_tenant) {
        auto it = sizes.find(kv.first);
        const uint64_t n = it == sizes.end() ? 0 : it->second;
        const unsigned __int128 tiles = ((unsigned __int128)n + m::kTileRows - 1) / m::kTileRows;
        want_items += tiles * ((kv.second + m::kQueryChunk - 1) / m::kQueryChunk);
    }
    if (rc != m::kPlanOk) {
        CHECK(p.items.empty());
        if (rc == m::kPlanTooManyItems) CHECK(want_items > m::kMaxItems);
        return;
    }
    CHECK(want_items <= m::kMaxItems);
    CHECK(p.item_count == (uint64_t)want_items && p.items.size() == (size_t)want_items);
    CHECK(p.perm.size() == nq && p.pos_seg.size() == nq);
    std::vector<int> seen(nq, 0);
    for (uint32_t q : p.perm) {
        CHECK(q < nq);
        seen[q]++;
    }
    for (int s : seen) CHECK(s == 1);
    CHECK(p.segs.size() == per_tenant.size() && p.seg_tenant.size() == p.segs.size());
    size_t at = 0;
    for (size_t s = 0; s < p.segs.size(); s++) {
        const m::Seg& g = p.segs[s];
        const uint32_t t = p.seg_tenant[s];
        if (s) CHECK(p.seg_tenant[s - 1] < t);
        CHECK(g.first == at && g.count == per_tenant[t] && g.count > 0);
        auto it = sizes.find(t);
        const uint64_t n = it == sizes.end() ? 0 : it->second;
        CHECK(g.n == n);
        if (n) CHECK(g.rows == fake(t, n).rows && g.ids == fake(t, n).ids);
        else CHECK(g.rows == nullptr && g.ids == nullptr);
        for (uint32_t j = 0; j < g.count; j++) {
            CHECK(tenants[p.perm[at + j]] == t);
            CHECK(p.pos_seg[at + j] == s);
            if (j) CHECK(p.perm[at + j - 1] < p.perm[at + j]);   // stable
        }
        at += g.count;
    }
    CHECK(at == nq);
    // coverage: per segment, a (tile, position) grid counted once each
    std::vector<std::vector<uint32_t>> cover(p.segs.size());
    if (count_pairs)
        for (size_t s = 0; s < p.segs.size(); s++) {
            const uint64_t tiles = (p.segs[s].n + m::kTileRows - 1) / m::kTileRows;
            cover[s].assign((size_t)tiles * p.segs[s].count, 0);
        }
    for (const m::Item& it : p.items) {
        CHECK(it.seg < p.segs.size());
        const m::Seg& g = p.segs[it.seg];
        CHECK(it.nq >= 1 && it.nq <= m::kQueryChunk && (uint64_t)it.q0 + it.nq <= g.count);
        CHECK((uint64_t)it.tile * m::kTileRows < g.n);
        if (count_pairs)
            for (uint32_t j = 0; j < it.nq; j++) cover[it.seg][(size_t)it.tile * g.count + it.q0 + j]++;
    }
    if (count_pairs)
        for (auto& c : cover)
            for (uint32_t v : c) CHECK(v == 1);   // every tile x position once: every (query, row) pair once
}

int main() {
    const uint32_t T = m::kTileRows, Q = m::kQueryChunk;
    run("nq = 0", {}, {{1, 10}}, m::kPlanOk);
    run("nq = 1", {7}, {{7, 5}}, m::kPlanOk);
    run("nq = 1, unknown tenant", {7}, {}, m::kPlanOk);
    run("all equal", std::vector<uint32_t>(100, 3), {{3, 2 * T + 3}}, m::kPlanOk);
    {
        std::vector<uint32_t> t;
        std::map<uint32_t, uint64_t> s;
        for (uint32_t i = 0; i < 500; i++) {
            t.push_back(1000 - i);
            s[1000 - i] = i % 7 == 0 ? 0 : i;
        }
        run("all distinct, descending, some empty", t, s, m::kPlanOk);
    }
    {
        // sizes at the T and Q edges
        std::vector<uint32_t> t;
        std::map<uint32_t, uint64_t> s;
        const uint64_t ns[] = {0, 1, T - 1, T, T + 1, 2 * T, 2 * T + 3};
        const uint32_t qs[] = {1, Q - 1, Q, Q + 1, 2 * Q, 2 * Q + 1};
        uint32_t tenant = 0;
        for (uint64_t n : ns)
            for (uint32_t q : qs) {
                s[tenant] = n;
                for (uint32_t j = 0; j < q; j++) t.push_back(tenant);
                tenant += 3;
            }
        std::mt19937 rng(5);
        for (size_t i = t.size(); i > 1; i--) std::swap(t[i - 1], t[rng() % i]);
        run("T and Q edges, shuffled", t, s, m::kPlanOk);
    }
    {
        std::mt19937 rng(11);
        for (int round = 0; round < 20; round++) {
            std::vector<uint32_t> t;
            std::map<uint32_t, uint64_t> s;
            const uint32_t tenants = 1 + rng() % 40, nq = rng() % 700;
            for (uint32_t i = 0; i < tenants; i++)
                if (rng() % 5) s[i * 0x01000193u] = rng() % (5 * T);
            for (uint32_t i = 0; i < nq; i++) t.push_back((rng() % tenants) * 0x01000193u);
            run("random", t, s, m::kPlanOk);
        }
    }
    run("tenant ids at the ends of u32", {0xffffffffu, 0, 0xffffffffu, 0x80000000u, 0}, {{0, 3}, {0xffffffffu, T + 1}, {0x80000000u, 1}},
        m::kPlanOk);
    // the refusals: 2^40 rows are 2^30 tiles, more work items than a 32-bit grid of 256-thread workgroups holds
    run("2^40 rows", {1, 2, 1}, {{1, 1ull << 40}, {2, 5}}, m::kPlanTooManyItems);
    run("2^63 rows x many queries", std::vector<uint32_t>(5000, 9), {{9, 1ull << 63}}, m::kPlanTooManyItems);
    // the largest item count that is accepted, and one more: 3 chunks x 2^22 tiles of tenant 4, the rest one query of tenant 5
    {
        std::vector<uint32_t> t(3 * Q, 4);
        t.push_back(5);
        const uint64_t big = (1ull << 32) - 1, tiles4 = (big + T - 1) / T, rest = m::kMaxItems - 3 * tiles4;
        run("kMaxItems", t, {{4, big}, {5, rest * T}}, m::kPlanOk, false);
        run("kMaxItems + 1", t, {{4, big}, {5, rest * T + 1}}, m::kPlanTooManyItems);
        t.push_back(4);   // a fourth chunk of tenant 4 alone
        run("one more chunk", t, {{4, big}}, m::kPlanTooManyItems);
    }
    // 2^32 rows are only 2^22 tiles: few enough items, but the histograms count a tenant's rows in 32 bits
    run("2^32 rows", {4}, {{4, 1ull << 32}}, m::kPlanTooManyRows);
    run("2^32 - 1 rows", {4}, {{4, (1ull << 32) - 1}}, m::kPlanOk, false);
    printf("ok %d checks\n", g_checks);
    return 0;
}
