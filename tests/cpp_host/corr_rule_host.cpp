// libwave_amd/csrc/wm_corr_rule.hpp away from any device, under the sanitizers: the hypothesis rule on degenerate,
// duplicate, non-finite and far-offset samples, the automatic sample distance and the refit from their sums.  The input
// file (argv[1]) is written by tests/test_corr_rule_host_cpu.py:
//     hyp p0 ... p8 q0 ... q8 min_d2                  (hex floats)
// Per line one goes out: "hyp flag t0 ... t11" (hex floats), which the test holds to the library's own evaluation.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>

#include "wm_corr_rule.hpp"

static int failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failed;                                                   \
        }                                                               \
    } while (0)

static bool all_zero(const float *T) {
    for (int i = 0; i < 12; ++i)
        if (T[i] != 0.f) return false;
    return true;
}

// |R R' - I| and det R of the twelve floats
static double ortho_error(const float *T, double *det) {
    double R[9], worst = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = T[i * 4 + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += R[i * 3 + k] * R[j * 3 + k];
            worst = std::fmax(worst, std::fabs(s - (i == j ? 1.0 : 0.0)));
        }
    *det = wm::det3(R);
    return worst;
}

static void fixed_cases() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    float T[12];
    const float q[9] = {1, 1, 1, 2, 1, 1, 1, 2, 1};
    {  // duplicates, all equal, collinear
        const float a[9] = {1, 2, 3, 1, 2, 3, 4, 5, 6}, b[9] = {1, 2, 3, 1, 2, 3, 1, 2, 3}, c[9] = {0, 0, 0, 1, 1, 1, 2, 2, 2};
        CHECK(wm::corr_hypothesis(a, q, 0.f, T) == wm::kCorrSkipped && all_zero(T));
        CHECK(wm::corr_hypothesis(b, q, 0.f, T) == wm::kCorrSkipped && all_zero(T));
        CHECK(wm::corr_hypothesis(c, q, 0.f, T) == wm::kCorrSkipped && all_zero(T));
    }
    {  // non-finite source points are skipped; non-finite TARGET points of a good sample give a non-finite entry: skipped
        float p[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
        for (int k = 0; k < 9; ++k)
            for (float bad : {nan, inf, -inf}) {
                float pp[9], qq[9];
                for (int i = 0; i < 9; ++i) pp[i] = p[i], qq[i] = q[i];
                pp[k] = bad;
                CHECK(wm::corr_hypothesis(pp, q, 0.f, T) == wm::kCorrSkipped && all_zero(T));
                qq[k] = bad;
                CHECK(wm::corr_hypothesis(p, qq, 0.f, T) == wm::kCorrSkipped && all_zero(T));
            }
        CHECK(wm::corr_hypothesis(p, q, nan, T) == wm::kCorrSkipped);
        CHECK(wm::corr_hypothesis(p, q, inf, T) == wm::kCorrSkipped);
        CHECK(wm::corr_hypothesis(p, q, 0.f, T) == wm::kCorrValid);
        CHECK(wm::corr_hypothesis(p, q, 1.f, T) == wm::kCorrSkipped);   // (|p1 - p0|^2 == 1 is not > 1)
        CHECK(wm::corr_hypothesis(p, q, 0.999f, T) == wm::kCorrValid);
    }
    {  // overflow and underflow of s
        const float big[9] = {0, 0, 0, 3e19f, 0, 0, 0, 3e19f, 0}, tiny[9] = {0, 0, 0, 1e-12f, 0, 0, 0, 1e-12f, 0};
        CHECK(wm::corr_hypothesis(big, q, 0.f, T) == wm::kCorrSkipped);
        CHECK(wm::corr_hypothesis(tiny, q, 0.f, T) == wm::kCorrSkipped);
    }
    {  // the identity, a pure shift, and the same 1e5 m away on both sides: a rotation that maps the sample
        for (float off : {0.f, 1.0e5f}) {
            float p[9] = {0, 0, 0, 4, 0, 0, 0, 3, 0}, qq[9];
            for (int i = 0; i < 9; ++i) p[i] += off;
            // q = Rz(90 deg) (p - off) + off + (1, 2, 3)
            for (int k = 0; k < 3; ++k) {
                const float x = p[3 * k] - off, y = p[3 * k + 1] - off, z = p[3 * k + 2] - off;
                qq[3 * k] = -y + off + 1.f;
                qq[3 * k + 1] = x + off + 2.f;
                qq[3 * k + 2] = z + off + 3.f;
            }
            CHECK(wm::corr_hypothesis(p, qq, 0.f, T) == wm::kCorrValid);
            double det;
            CHECK(ortho_error(T, &det) <= 1e-6 && det > 0.999);
            // the double work on uncentred sums loses |offset|^2 * 2^-53 of the cross sums: ~1e-6 of the rotation at 1e5 m
            const double tol = off == 0.f ? 1e-6 : 2e-5;
            CHECK(std::fabs(T[0]) <= tol && std::fabs(T[1] + 1.f) <= tol && std::fabs(T[4] - 1.f) <= tol && std::fabs(T[10] - 1.f) <= tol);
            for (int k = 0; k < 3; ++k) {
                const float d2 = wm::corr_pair_d2(T, p[3 * k], p[3 * k + 1], p[3 * k + 2], qq[3 * k], qq[3 * k + 1], qq[3 * k + 2]);
                CHECK(d2 <= (off == 0.f ? 1e-10f : 1.f));  // (a float at 1e5 m has 8 mm steps, the transform's t carries |R| * 1e5)
            }
        }
    }
    {  // the automatic sample distance: a 3-4-5 box of eight corners; its clamp on a flat set; poison and non-finite sums
        double sum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        int n = 0;
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j)
                for (int k = 0; k < 2; ++k, ++n) {
                    const double d[3] = {3.0 * i, 4.0 * j, 5.0 * k};
                    for (int a = 0; a < 3; ++a) sum[a] += d[a];
                    sum[3] += d[0] * d[0], sum[4] += d[0] * d[1], sum[5] += d[0] * d[2];
                    sum[6] += d[1] * d[1], sum[7] += d[1] * d[2], sum[8] += d[2] * d[2];
                }
        const double want = ((1.5 + 2.0 + 2.5) / 3.0) * ((1.5 + 2.0 + 2.5) / 3.0);  // (the eigenvalues are 2.25, 4, 6.25)
        CHECK(std::fabs((double) wm::corr_min_d2_from_sums(sum, false, n) - want) <= 1e-6);
        CHECK(wm::corr_min_d2_from_sums(sum, true, n) == 0.f);
        double flat[9] = {8, 0, 0, 16, 0, 0, 0, 0, 0};  // eight points at x = 0 / 2: variance 1 along x only
        CHECK(std::fabs((double) wm::corr_min_d2_from_sums(flat, false, 8) - 1.0 / 9.0) <= 1e-7);
        double zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        CHECK(wm::corr_min_d2_from_sums(zero, false, 8) == 0.f);
        sum[4] = std::numeric_limits<double>::quiet_NaN();
        CHECK(wm::corr_min_d2_from_sums(sum, false, n) == 0.f);
        sum[4] = std::numeric_limits<double>::infinity();
        CHECK(wm::corr_min_d2_from_sums(sum, false, n) == 0.f);
    }
    {  // the refit from sums relative to (p0, q0) 1e5 m away: four pairs under Rz(90 deg) and a shift
        const float p0[3] = {1.0e5f, 1.0e5f, 1.0e5f}, q0[3] = {1.0e5f + 1.f, 1.0e5f + 2.f, 1.0e5f + 3.f};
        const double dp[4][3] = {{0, 0, 0}, {4, 0, 0}, {0, 3, 0}, {0, 0, 2}};
        double sum[wm::kCorrRefitComps] = {0};
        for (auto &d : dp) {
            const double dq[3] = {-d[1], d[0], d[2]};
            for (int a = 0; a < 3; ++a) {
                sum[a] += d[a];
                sum[3 + a] += dq[a];
                for (int b = 0; b < 3; ++b) sum[6 + a * 3 + b] += dq[a] * d[b];
            }
        }
        double T[16];
        CHECK(wm::corr_refit_from_sums(sum, false, 4.0, p0, q0, T));
        CHECK(std::fabs(T[0]) <= 1e-12 && std::fabs(T[1] + 1) <= 1e-12 && std::fabs(T[4] - 1) <= 1e-12 && std::fabs(T[10] - 1) <= 1e-12);
        // t = q0 - R p0 = (q0x + p0y, q0y - p0x, q0z - p0z)
        CHECK(std::fabs(T[3] - ((double) q0[0] + (double) p0[1])) <= 1e-9 && std::fabs(T[7] - ((double) q0[1] - (double) p0[0])) <= 1e-9 &&
              std::fabs(T[11] - 3.0) <= 1e-9 && T[15] == 1.0);
        CHECK(!wm::corr_refit_from_sums(sum, true, 4.0, p0, q0, T));
        CHECK(!wm::corr_refit_from_sums(sum, false, 2.0, p0, q0, T));
        sum[7] = std::numeric_limits<double>::quiet_NaN();
        CHECK(!wm::corr_refit_from_sums(sum, false, 4.0, p0, q0, T));
    }
}

int main(int argc, char **argv) {
    fixed_cases();
    if (argc >= 2) {
        std::ifstream in(argv[1]);
        if (!in) return 3;
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ss(line);
            std::string tag, tok;
            ss >> tag;
            if (tag != "hyp") continue;
            float v[19];
            int n = 0;
            while (n < 19 && ss >> tok) v[n++] = std::strtof(tok.c_str(), nullptr);
            CHECK(n == 19);
            if (n != 19) continue;
            float T[12];
            const unsigned flag = wm::corr_hypothesis(v, v + 9, v[18], T);
            std::printf("hyp %u", flag);
            for (int i = 0; i < 12; ++i) std::printf(" %a", (double) T[i]);
            std::printf("\n");
        }
    }
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
