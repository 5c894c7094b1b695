// libwave_amd/csrc/wm_sac_walk.hpp away from any device: PCL's loop walked over recorded (flag, count) sequences cut
// into rounds of several sizes, and the plane of the refit's nine sums.  The input file (argv[1]) is written by
// tests/test_sac_walk_host_cpu.py:
//     walk NAME n max_iterations probability L        followed by L lines "flag count"
//     sums m p0x p0y p0z a b c d s0 ... s8            (hex floats)
// Per walk and cut one line goes out: NAME cut iterations skipped hypotheses best_entry best_count rounds; per sums
// line the returned plane.  A walk that asks for entries the file does not hold is a failed check.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "wm_sac_walk.hpp"

static int failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failed;                                                   \
        }                                                               \
    } while (0)

static void walk(const std::string &name, size_t n, int max_it, double prob, const std::vector<unsigned> &flags,
                 const std::vector<unsigned> &counts) {
    const unsigned cuts[] = {1u, 7u, 256u, 1024u};
    wm::SacWalk first;
    for (unsigned cut : cuts) {
        wm::SacWalk w;
        w.start(max_it, prob, n);
        CHECK(w.going);
        bool enough = true;
        while (w.going) {
            const unsigned R = w.round_size(cut);
            CHECK(R >= 1 && R <= cut && (long long) R <= (long long) max_it + 1 - w.it);
            if (w.j + R > flags.size()) {
                enough = false;
                break;
            }
            const unsigned long long j0 = w.j;
            unsigned best_seen = 0;
            w.feed_round(flags.data() + j0, counts.data() + j0, R, [&](unsigned e) { best_seen = e + 1; });
            CHECK(w.j > j0 && w.j <= j0 + R);          // a round consumes at least one entry and never more than it holds
            CHECK(w.going ? w.j == j0 + R : true);     // a walk that goes on has consumed the whole round
            if (best_seen) CHECK(w.best_j >= (long long) j0 && w.best_j < (long long) (j0 + R));
        }
        CHECK(enough);
        std::printf("%s %u %lld %lld %llu %lld %lld %d\n", name.c_str(), cut, w.it, w.skipped, w.j, w.best_j, w.best, w.rounds);
        if (cut == cuts[0]) first = w;
        CHECK(w.it == first.it && w.skipped == first.skipped && w.j == first.j && w.best_j == first.best_j &&
              w.best == first.best && w.k == first.k);
    }
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 3;
    std::string line;
    int walks = 0, sums = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string kind;
        ss >> kind;
        if (kind == "walk") {
            std::string name;
            size_t n = 0, L = 0;
            int max_it = 0;
            double prob = 0;
            ss >> name >> n >> max_it >> prob >> L;
            std::vector<unsigned> flags(L), counts(L);
            for (size_t i = 0; i < L; ++i) {
                if (!std::getline(in, line)) return 4;
                if (std::sscanf(line.c_str(), "%u %u", &flags[i], &counts[i]) != 2) return 4;
            }
            walk(name, n, max_it, prob, flags, counts);
            ++walks;
        } else if (kind == "sums") {
            std::string tok;
            std::vector<double> v;
            while (ss >> tok) v.push_back(std::strtod(tok.c_str(), nullptr));
            if (v.size() != 17) return 5;
            const float p0[3] = {(float) v[1], (float) v[2], (float) v[3]};
            const float model[4] = {(float) v[4], (float) v[5], (float) v[6], (float) v[7]};
            float out[4] = {0, 0, 0, 0};
            CHECK(wm::sac_plane_from_sums(v.data() + 8, false, p0, v[0], model, out));
            std::printf("plane %a %a %a %a\n", (double) out[0], (double) out[1], (double) out[2], (double) out[3]);
            float keep[4] = {7, 7, 7, 7};
            CHECK(!wm::sac_plane_from_sums(v.data() + 8, true, p0, v[0], model, keep) && keep[0] == 7);  // poisoned: the model stays
            const float flipped[4] = {-model[0], -model[1], -model[2], -model[3]};
            float neg[4];
            CHECK(wm::sac_plane_from_sums(v.data() + 8, false, p0, v[0], flipped, neg));
            CHECK(neg[0] == -out[0] && neg[1] == -out[1] && neg[2] == -out[2] && neg[3] == -out[3]);  // the sign is the model's
            ++sums;
        }
    }
    CHECK(walks > 0 && sums > 0);
    CHECK(wm::sac_threshold(0.25) == 0.25f && (double) wm::sac_threshold(0.05) >= 0.05 &&
          (double) nextafterf(wm::sac_threshold(0.05), 0.f) < 0.05);
    CHECK(wm::sac_toward_zero(1.0) == 1.0f && (double) wm::sac_toward_zero(0.1) <= 0.1 && (double) wm::sac_toward_zero(-0.1) >= -0.1);
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
