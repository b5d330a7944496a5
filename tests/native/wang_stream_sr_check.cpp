// wang_stream_sr_check.cpp -- the integer rule of the resampling Wang / Panako stream sets (ucfp_amd/csrc/stream_resample.h,
// DESIGN.md A21) driven on a CPU: random feeds cut at random through rs_span, every read of the assemble step done on
// heap buffers of EXACTLY the sizes the device holds (a slot's carry of carry_cap floats, a chunk of its own length),
// every carried input moved as the save step moves it.  The assembled samples must equal the offline resampler's over
// the whole feed bit for bit.  Build and run under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined wang_stream_sr_check.cpp -o wang_stream_sr_check && ./wang_stream_sr_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../ucfp_amd/csrc/stream_resample.h"

using namespace ucfp::wstreams;

static int fails = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            if (fails++ < 20) {                         \
                std::printf("FAIL %s: ", #c);           \
                std::printf(__VA_ARGS__);               \
                std::printf("\n");                      \
            }                                           \
        }                                               \
    } while (0)

// A1 over a whole clip, as the offline entries compute it
static std::vector<float> offline(const std::vector<float>& x, uint32_t sr) {
    const uint64_t n = x.size(), m = n * kSr8k / sr;
    std::vector<float> out(m);
    for (uint64_t i = 0; i < m; i++) {
        const uint64_t num = i * sr, idx = num / kSr8k;
        const float frac = (float)((double)(uint32_t)(num % kSr8k) / (double)kSr8k);
        const float x0 = x[idx], x1 = x[idx + 1 < n ? idx + 1 : n - 1];
        const float d = x1 - x0;
        const float mm = d * frac;
        out[i] = x0 + mm;
    }
    return out;
}

// one stream: the slot's carry buffer and the push of one chunk, reading as the assemble kernel does
struct Stream {
    uint32_t sr, cap;
    uint64_t n = 0;
    float* carry;
    explicit Stream(uint32_t r) : sr(r), cap(carry_cap_of(r)), carry(new float[carry_cap_of(r) ? carry_cap_of(r) : 1]) {}
    ~Stream() { delete[] carry; }
    float input(const RsSpan& e, const float* chunk, uint64_t a) const {
        return a < e.n0 ? carry[a - e.c_in] : chunk[a - e.n0];
    }
    void push(const float* feed, uint64_t m, bool fin, std::vector<float>* out) {
        float* chunk = new float[m ? m : 1];           // exactly the chunk: a read past it is caught
        if (m) std::memcpy(chunk, feed + n, m * 4);
        const RsSpan e = rs_span(n, m, sr, fin);
        CHECK(e.s1 >= e.s0 && e.c_in <= e.n0 && e.n0 - e.c_in <= cap, "span in: n0 %llu m %llu sr %u",
              (unsigned long long)n, (unsigned long long)m, sr);
        CHECK(e.c_out >= e.c_in && e.c_out <= e.n1 && e.n1 - e.c_out <= cap, "span out: n0 %llu m %llu sr %u",
              (unsigned long long)n, (unsigned long long)m, sr);
        for (uint64_t o = e.s0; o < e.s1; o++) {
            const uint64_t num = o * sr, idx = num / kSr8k;
            const float frac = (float)((double)(uint32_t)(num % kSr8k) / (double)kSr8k);
            uint64_t a1 = idx + 1;
            if (fin && a1 >= e.n1) a1 = e.n1 - 1;
            CHECK(idx >= e.c_in && a1 < e.n1, "read: o %llu sr %u", (unsigned long long)o, sr);
            const float x0 = input(e, chunk, idx), x1 = input(e, chunk, a1);
            const float d = x1 - x0;
            const float mm = d * frac;
            out->push_back(x0 + mm);
        }
        if (!fin) {                                    // save: read, then write (the inputs may move inside the buffer)
            std::vector<float> v;
            for (uint64_t a = e.c_out; a < e.n1; a++) v.push_back(input(e, chunk, a));
            for (size_t i = 0; i < v.size(); i++) carry[i] = v[i];
        }
        n = e.n1;
        delete[] chunk;
    }
};

int main() {
    const uint32_t rates[] = {1000, 1001, 4000, 7999, 8001, 11025, 16000, 22050, 44100, 48000, 96000, 383999, 384000};
    std::mt19937_64 rng(21);
    uint64_t pushes = 0;
    for (uint32_t sr : rates) {
        CHECK(sr_ok(sr) && carry_cap_of(sr) == (sr + 7999) / 8000 + 1, "cap %u", sr);
        for (int trial = 0; trial < 6; trial++) {
            const uint64_t len = trial == 0 ? 0 : trial == 1 ? 1 : (uint64_t)(sr * (0.05 + 0.25 * (rng() % 100) / 100.0));
            std::vector<float> x(len);
            for (auto& v : x) v = (float)((double)(rng() % 2000001) / 1000000.0 - 1.0);
            const std::vector<float> want = offline(x, sr);
            for (int fin_carries = 0; fin_carries < 2; fin_carries++) {
                Stream st(sr);
                std::vector<float> got;
                uint64_t a = 0;
                const uint32_t k = (sr + 7999) / 8000;
                while (a < len) {
                    const uint64_t pick[] = {0, 1, 1, 2, k - 1, k, k + 1, 127, 997, sr / 10, rng() % (sr / 2 + 1)};
                    uint64_t c = trial == 2 ? 1 : pick[rng() % 11];
                    if (c > len - a) c = len - a;
                    const bool last = fin_carries && a + c == len;
                    st.push(x.data(), c, last, &got);
                    pushes++;
                    a += c;
                    if (last) break;
                    CHECK(got.size() == samples_of(a, sr, false), "S: %llu sr %u", (unsigned long long)a, sr);
                }
                if (!(fin_carries && len)) st.push(x.data(), 0, true, &got);
                CHECK(got.size() == want.size() && (got.empty() || !std::memcmp(got.data(), want.data(), got.size() * 4)),
                      "feed of %llu at %u differs", (unsigned long long)len, sr);
            }
        }
    }
    {   // one long push: two seconds at 384 kHz behind a five-sample one
        const uint32_t sr = 384000;
        std::vector<float> x(2 * sr + 17);
        for (auto& v : x) v = (float)((double)(rng() % 2000001) / 1000000.0 - 1.0);
        const std::vector<float> want = offline(x, sr);
        Stream st(sr);
        std::vector<float> got;
        st.push(x.data(), 5, false, &got);
        st.push(x.data(), x.size() - 5, true, &got);
        CHECK(want.size() >= 16000 && got.size() == want.size() && !std::memcmp(got.data(), want.data(), got.size() * 4),
              "long push at %u differs", sr);
    }
    for (int i = 0; i < 200000; i++) {   // the 64-bit and the 128-bit form of the rule agree, on both sides of 2^50 / 2^44
        const uint32_t sr = kMinSr + (uint32_t)(rng() % (kMaxSr - kMinSr + 1));
        const uint64_t n = (i & 1) ? (rng() >> (rng() % 60)) : ((uint64_t)1 << 50) - 100 + rng() % 200;
        const unsigned __int128 k = kSr8k;
        const uint64_t len = (uint64_t)(n * k / sr), nb = n ? (uint64_t)(((n - 1) * k + sr - 1) / sr) : 0;
        if (sr != kSr8k) {
            CHECK(samples_of(n, sr, true) == len && samples_of(n, sr, false) == (nb < len ? nb : len), "S(%llu) at %u",
                  (unsigned long long)n, sr);
        }
        const uint64_t s = (i & 1) ? (rng() >> (4 + rng() % 56)) : ((uint64_t)1 << 44) - 100 + rng() % 200;
        CHECK(carry_from(s, sr) == (uint64_t)((unsigned __int128)s * sr / kSr8k), "carry_from(%llu) at %u",
              (unsigned long long)s, sr);
    }
    {
        const RsSpan e = rs_span(12345, 678, kSr8k, false);
        CHECK(e.s0 == 12345 && e.c_in == 12345 && e.s1 == 13023 && e.c_out == 13023, "8 kHz span");
    }
    CHECK(!sr_ok(999) && !sr_ok(384001) && sr_ok(8000) && carry_cap_of(8000) == 0, "range");
    CHECK(samples_of(~0ull, 384000, true) == (uint64_t)(((unsigned __int128)~0ull * 8000) / 384000), "wide");
    if (fails) return 1;
    std::printf("ok %llu pushes\n", (unsigned long long)pushes);
    return 0;
}
