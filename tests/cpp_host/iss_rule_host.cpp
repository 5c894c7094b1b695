// The saliency step of wm_iss_keypoints (libwave_amd/csrc/wm_iss_rule.hpp) on the host, away from any device: built by
// tests/test_iss_rule_host_cpu.py with g++ -fsanitize=address,undefined -ffp-contract=off.  It makes its own checks on
// zero, huge, negative-definite and rank-deficient sums, then reads lines "thr s0 ... s5 n_s x g21 g32 min_nb" from
// the file given as its argument and prints "thr <hex double>" for each, which the test holds to wm_iss_third.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include "wm_iss_rule.hpp"

static int failed = 0;
#define CHECK(cond)                                            \
    do {                                                       \
        if (!(cond)) {                                         \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failed;                                          \
        }                                                      \
    } while (0)

static double third(long long xx, long long xy, long long xz, long long yy, long long yz, long long zz, int n_s = 10, int min_nb = 5,
                    int x = 0, double g21 = 0.975, double g32 = 0.975) {
    const long long s[6] = {xx, xy, xz, yy, yz, zz};
    return wm::iss_third(s, n_s, min_nb, x, g21, g32);
}

int main(int argc, char **argv) {
    // zero sums: l1 = 0, 0 / 0 is a NaN and l3 > 0 fails first
    CHECK(third(0, 0, 0, 0, 0, 0) == 0.0);
    // a clean diagonal: l = 4, 2, 1 (scaled by 2^36 at x = 0): ratios 0.5, third = l3 2^-36
    {
        const long long u = 1ll << 36;
        CHECK(third(4 * u, 0, 0, 2 * u, 0, u) == 1.0);
        CHECK(third(u, 0, 0, 4 * u, 0, 2 * u) == 1.0);   // (the order of the axes does not matter)
        CHECK(third(4 * u, 0, 0, 2 * u, 0, u, 10, 5, 3) == 8.0);  // x: the cloud's units
        CHECK(third(4 * u, 0, 0, 2 * u, 0, u, 4, 5) == 0.0);      // too few neighbours
        CHECK(third(4 * u, 0, 0, 2 * u, 0, u, 5, 5) == 1.0);
        CHECK(third(4 * u, 0, 0, 2 * u, 0, u, 10, 5, 0, 0.5, 0.975) == 0.0);  // l2 / l1 == gamma_21: strict
        CHECK(third(4 * u, 0, 0, 2 * u, 0, u, 10, 5, 0, 0.975, 0.5) == 0.0);
        CHECK(third(4 * u, 0, 0, 2 * u, 0, u, 10, 5, 0, 0.0, 0.0) == 0.0);    // gamma = 0 gives none
        CHECK(third(u, 0, 0, u, 0, u) == 0.0);                                 // a ball: ratios 1
    }
    // rank deficient (a plane, a line): l3 == 0 exactly
    CHECK(third(1000, 0, 0, 500, 0, 0) == 0.0);
    CHECK(third(1000, 1000, 0, 1000, 0, 0) == 0.0);
    // negative definite and indefinite: never salient
    CHECK(third(-4000, 0, 0, -2000, 0, -1000) == 0.0);
    CHECK(third(4000, 0, 0, 2000, 0, -1) == 0.0);
    // huge sums: finite doubles, no overflow of anything
    {
        const long long h = LLONG_MAX;
        const double t = third(h, 0, 0, h / 2, 0, h / 4);
        CHECK(t > 0.0 && t - t == 0.0);
        CHECK(third(h, h, h, h, h, h) == 0.0 || third(h, h, h, h, h, h) > 0.0);  // (runs; rank 1 up to rounding)
        CHECK(third(LLONG_MIN, 0, 0, LLONG_MIN, 0, LLONG_MIN) == 0.0);
        CHECK(third(h, LLONG_MIN, h, h, LLONG_MIN, h) - third(h, LLONG_MIN, h, h, LLONG_MIN, h) == 0.0);
    }
    // the extreme exponents
    {
        const long long u = 1ll << 36;
        const double lo = third(4 * u, 0, 0, 2 * u, 0, u, 10, 5, -125), hi = third(4 * u, 0, 0, 2 * u, 0, u, 10, 5, 128);
        CHECK(lo == ldexp(1.0, -125) && hi == ldexp(1.0, 128));
    }
    if (argc > 1) {
        FILE *f = fopen(argv[1], "r");
        if (!f) {
            printf("cannot open %s\n", argv[1]);
            return 2;
        }
        long long s[6];
        int n_s, x, min_nb;
        double g21, g32;
        while (fscanf(f, " thr %lld %lld %lld %lld %lld %lld %d %d %la %la %d", &s[0], &s[1], &s[2], &s[3], &s[4], &s[5], &n_s, &x,
                      &g21, &g32, &min_nb) == 11)
            printf("thr %a\n", wm::iss_third(s, n_s, min_nb, x, g21, g32));
        fclose(f);
    }
    printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
