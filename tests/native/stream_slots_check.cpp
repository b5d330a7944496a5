// stream_slots_check.cpp -- the slot table of the stream sets (ucfp_amd/csrc/stream_slots.h) against a naive model, on
// a CPU, meant to be built with -fsanitize=address,undefined.  Random acquires, releases and slot lists (duplicates,
// closed slots, slots out of range, lists longer than the set) on sets of 1, 2 and 64 slots: the table must give the
// model's verdict and message, hand out the lowest free slot with nothing seen, and leave `seen` all zero after every
// operation, refused ones included.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined stream_slots_check.cpp -o stream_slots_check && ./stream_slots_check
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "../../ucfp_amd/csrc/stream_slots.h"

static std::string g_last;

namespace ucfp {
int capi_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last = buf;
    return code;
}
}  // namespace ucfp

namespace {

std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

#define REQUIRE(cond, ...)                                   \
    do {                                                     \
        if (!(cond)) {                                       \
            fprintf(stderr, "line %d: %s: ", __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                    \
            fprintf(stderr, "\n");                           \
            exit(1);                                         \
        }                                                    \
    } while (0)

struct Model {
    uint32_t max;
    std::vector<bool> open;
    std::vector<uint64_t> n;

    // the first refusal of a list, "" when it passes; `stop`: entries judged before a refusal of the caller's own
    std::string judge(const std::vector<uint32_t>& l, const char* what, size_t stop) const {
        std::vector<bool> named(max, false);
        for (size_t i = 0; i < l.size() && i < stop; i++) {
            const uint32_t s = l[i];
            if (s >= max) return fmt("slot %u out of range [0, %u)", s, max);
            if (!open[s]) return fmt("slot %u is not open", s);
            if (named[s]) return fmt("slot %u appears twice in one %s", s, what);
            named[s] = true;
        }
        return "";
    }
};

void same_state(const ucfp::streams::Slots& t, const Model& m, const char* after) {
    for (uint32_t i = 0; i < m.max; i++) {
        REQUIRE(t.seen[i] == 0, "seen[%u] set after %s", i, after);
        REQUIRE((t.open[i] != 0) == m.open[i], "open[%u] differs after %s", i, after);
        REQUIRE(t.n[i] == m.n[i], "n[%u] differs after %s", i, after);
    }
}

void expect(int rc, const std::string& want, const char* op) {
    if (want.empty()) {
        REQUIRE(rc == UCFP_OK, "%s refused (%s), the model accepts", op, g_last.c_str());
    } else {
        REQUIRE(rc == UCFP_E_INVALID, "%s gave %d, the model refuses with \"%s\"", op, rc, want.c_str());
        REQUIRE(g_last == want, "%s said \"%s\", the model \"%s\"", op, g_last.c_str(), want.c_str());
    }
}

size_t run(uint32_t max, size_t ops, uint64_t seed) {
    std::mt19937_64 rng(seed);
    auto below = [&](uint64_t k) { return (uint64_t)(rng() % k); };
    ucfp::streams::Slots t;
    t.init(max);
    Model m{max, std::vector<bool>(max, false), std::vector<uint64_t>(max, 0)};
    same_state(t, m, "init");
    size_t refused = 0;
    for (size_t op = 0; op < ops; op++) {
        const uint64_t kind = below(10);
        if (kind < 2) {                                               // acquire
            uint32_t want = 0;
            while (want < max && m.open[want]) want++;
            uint32_t got = 0xdeadbeefu;
            const int rc = t.acquire(&got);
            if (want == max) {
                expect(rc, fmt("all %u slots are open", max), "acquire");
                refused++;
            } else {
                expect(rc, "", "acquire");
                REQUIRE(got == want, "acquire gave slot %u, the lowest free one is %u", got, want);
                m.open[want] = true;
                m.n[want] = 0;                                        // whatever the slot saw before
            }
            same_state(t, m, "acquire");
        } else if (kind < 4) {                                        // release: now and then out of range
            const uint32_t s = below(8) == 0 ? max + (uint32_t)below(3) : (uint32_t)below(max);
            const int rc = t.release(s);
            if (s >= max || !m.open[s]) {
                expect(rc, fmt("slot %u is not open", s), "release");
                refused++;
            } else {
                expect(rc, "", "release");
                m.open[s] = false;
                m.n[s] = 0;
            }
            same_state(t, m, "release");
        } else {                                                      // a list, judged whole or entry by entry
            const size_t len = below(6) == 0 ? max + 1 + below(3) : below((uint64_t)max + 1);
            std::vector<uint32_t> l(len);
            for (auto& s : l) {
                const uint64_t r = below(16);
                s = r == 0 ? max + (uint32_t)below(4) : r == 1 ? 0xffffffffu : (uint32_t)below(max);
            }
            if (len >= 2 && below(3) == 0) l[below(len)] = l[below(len)];   // a duplicate, unless both picks coincide
            const bool whole = kind < 7;
            const char* what = whole ? "call" : "push";
            std::string want = len > max ? fmt("%zu entries in one %s, the set has %u slots", len, what, max) : "";
            int rc;
            if (whole) {
                if (want.empty()) want = m.judge(l, what, len);
                rc = t.check(l.data(), len, "entries", what);
            } else {
                // as the Wang and text planners: the caller's own check of an entry follows its mark and may refuse
                const size_t own = below(4) == 0 && len ? below(len) : len;
                rc = t.fits(len, "entries", what);
                if (rc == UCFP_OK) {
                    for (size_t i = 0; i < len; i++) {
                        rc = t.mark(l[i], what);
                        if (rc == UCFP_OK && i == own) rc = ucfp::capi_fail(UCFP_E_INVALID, "entry %zu is too large", i);
                        if (rc) break;
                    }
                    t.unmark(l.data(), len);
                }
                if (want.empty()) want = m.judge(l, what, own + 1);
                if (want.empty() && own < len) want = fmt("entry %zu is too large", own);
            }
            expect(rc, want, whole ? "check" : "mark");
            refused += !want.empty();
            if (want.empty())                                         // an accepted push advances its slots
                for (uint32_t s : l) t.n[s] = m.n[s] = m.n[s] + 1 + below(1000);
            same_state(t, m, "a list");
        }
    }
    return refused;
}

}  // namespace

int main(int argc, char** argv) {
    const size_t ops = argc > 1 ? strtoull(argv[1], nullptr, 10) : 120000;
    size_t refused = 0;
    for (uint32_t max : {1u, 2u, 64u}) refused += run(max, ops, 0x5107u + max);
    REQUIRE(refused > ops / 10 && refused < 3 * ops - ops / 10, "%zu of %zu operations refused: the mix is off", refused, 3 * ops);
    printf("ok: %zu operations on sets of 1, 2 and 64 slots, %zu refused\n", 3 * ops, refused);
    return 0;
}
