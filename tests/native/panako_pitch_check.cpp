// Runs the A22 pieces of ucfp_amd/csrc/panako_match.h on the CPU for tests/test_panako_pitch_spec.py.
// stdin, one case per line:  scale_min scale_max scale_step window slack r_slack bins f_slack  h d h' d'  k k' s
// stdout, one line per case: ok nh  B_s(k)  jlo jhi of the bin (k, k')  jlo jhi of the match  k'_lo k'_hi of bin k over all
//                            hypotheses
// (jlo > jhi = no hypothesis, k'_lo > k'_hi = no bin).  A plan that the old check accepts with bins = f_slack = 0 must
// be the same plan; a mismatch ends the run.
#include <cstdio>
#include <cstdlib>

#include "../../ucfp_amd/csrc/panako_match.h"

using namespace ucfp;

#define REQUIRE(x)                                              \
    do {                                                        \
        if (!(x)) {                                             \
            fprintf(stderr, "line %ld: %s\n", line, #x);        \
            return 2;                                           \
        }                                                       \
    } while (0)

int main() {
    unsigned smin, smax, step, win, slack, rs, bins, f, h, d, hp, dp, k, kp, s;
    long line = 0;
    while (scanf("%u %u %u %u %u %u %u %u %u %u %u %u %u %u %u", &smin, &smax, &step, &win, &slack, &rs, &bins, &f, &h, &d, &hp,
                 &dp, &k, &kp, &s) == 15) {
        line++;
        PkMatch m, old;
        if (!pk_plan_ex(smin, smax, step, win, slack, rs, bins, f, &m)) {
            puts("0");
            continue;
        }
        REQUIRE(pk_plan(smin, smax, step, win, slack, rs, &old));
        REQUIRE(old.smin == m.smin && old.step == m.step && old.nh == m.nh && old.window == m.window && old.slack == m.slack &&
                old.r_slack == m.r_slack && old.bins == 0 && old.f_slack == 0);
        int32_t blo, bhi, jlo, jhi, klo, khi;
        pk_bin_interval(m, (int32_t)k, (int32_t)kp, m.f_slack, &blo, &bhi);
        pk_interval_scaled(m, h, (int32_t)d, hp, (int32_t)dp, &jlo, &jhi);
        pk_bin_range(m, (int32_t)k, 0, m.nh - 1, &klo, &khi);
        REQUIRE(klo >= 0 && khi <= kPkMaxBin);
        printf("1 %d %d %d %d %d %d %d %d\n", m.nh, pk_bin((int32_t)s, (int32_t)k), blo, bhi, jlo, jhi, klo, khi);
    }
    return 0;
}
