// Runs the integer pieces of ucfp_amd/csrc/panako_match.h on the CPU for tests/test_panako_match_spec.py.
// stdin, one case per line:  scale_min scale_max scale_step window slack r_slack  h a d a' d'  ord1 cnt1 j1 off1  ord2 cnt2 j2 off2
// stdout, one line per case: ok nh  first_probe n_probes  jlo jhi  offset(jlo) offset(jhi)  rank(j1) rank(j2)
//                            cmp(best1, best2) cmp(vote1, vote2) past_window(vote2, vote1)
// (jlo > jhi = no hypothesis; offsets 0 then).  Every packed value is also unpacked again; a mismatch ends the run.
#include <cstdio>
#include <cstdlib>

#include "../../ucfp_amd/csrc/panako_match.h"

using namespace ucfp;

static int cmp(uint64_t a, uint64_t b) { return a < b ? -1 : a > b ? 1 : 0; }

#define REQUIRE(x)                                              \
    do {                                                        \
        if (!(x)) {                                             \
            fprintf(stderr, "line %ld: %s\n", line, #x);        \
            return 2;                                           \
        }                                                       \
    } while (0)

int main() {
    unsigned smin, smax, step, win, slack, rs, h, a, d, ap, dp, o1, c1, j1, o2, c2, j2;
    int f1, f2;
    long line = 0;
    while (scanf("%u %u %u %u %u %u %u %u %u %u %u %u %u %u %d %u %u %u %d", &smin, &smax, &step, &win, &slack, &rs, &h, &a, &d,
                 &ap, &dp, &o1, &c1, &j1, &f1, &o2, &c2, &j2, &f2) == 19) {
        line++;
        PkMatch m;
        if (!pk_plan(smin, smax, step, win, slack, rs, &m)) {
            puts("0");
            continue;
        }
        uint32_t first, np;
        pk_probes(h, m.r_slack, &first, &np);
        int32_t jlo, jhi;
        pk_interval(m, (int32_t)d, (int32_t)dp, &jlo, &jhi);
        const bool any = jlo <= jhi;
        const int32_t off_lo = any ? pk_offset(m.smin + jlo * m.step, a, ap) : 0;
        const int32_t off_hi = any ? pk_offset(m.smin + jhi * m.step, a, ap) : 0;
        const uint32_t r1 = pk_pref_rank(m, (int32_t)j1), r2 = pk_pref_rank(m, (int32_t)j2);
        const uint64_t b1 = pk_best(c1, r1, f1), b2 = pk_best(c2, r2, f2);
        const uint64_t v1 = pk_vote_key(o1, j1, f1), v2 = pk_vote_key(o2, j2, f2);
        REQUIRE(pk_best_count(b1) == c1 && pk_best_rank(b1) == r1 && pk_best_delta(b1) == f1);
        REQUIRE(pk_vote_ord(v1) == o1 && pk_vote_j(v1) == j1 && pk_vote_delta(v1) == f1);
        const uint64_t e = pk_entry(o1, ap, dp);
        REQUIRE(pk_entry_ord(e) == o1 && pk_entry_a(e) == ap && pk_entry_d(e) == dp);
        printf("1 %d %u %u %d %d %d %d %u %u %d %d %d\n", m.nh, first, np, jlo, jhi, off_lo, off_hi, r1, r2, cmp(b1, b2),
               cmp(v1, v2), pk_past_window(v2, v1, (uint32_t)m.window) ? 1 : 0);
    }
    return 0;
}
