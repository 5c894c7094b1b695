// The C++ drop-in away from any device: the YAML constructor reads the reference's 14 keys, a missing file keeps
// the defaults, and a GroundSegmentation is constructed, configured and copied without opening a device.
#include <cstdio>

#include "wave/matching/ground_segmentation.hpp"

static int failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failed;                                                   \
        }                                                               \
    } while (0)

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    wave::GroundSegmentationParams d{};
    CHECK(d.rmax == 100 && d.max_bin_points == 200 && d.num_seed_points == 10 && d.p_l == 4.f && d.p_sf == 1.f);
    CHECK(d.p_sn == 0.3f && d.p_tmodel == 5.f && d.p_tdata == 5.f && d.p_tg == 0.3f && d.robot_height == 1.2);
    CHECK(d.max_seed_range == 50 && d.max_seed_height == 15 && d.num_bins_a == 72 && d.num_bins_l == 200);
    wave::GroundSegmentationParams y{std::string(argv[1])};
    CHECK(y.p_l == 10.f && y.rmax == 100 && y.num_bins_a == 72 && y.num_bins_l == 200 && y.num_seed_points == 10);
    CHECK(y.p_sn == 0.3f && y.p_tg == 0.3f && y.robot_height == 1.2 && y.max_seed_range == 50);
    wave::GroundSegmentationParams missing{std::string("/nonexistent/ground.yaml")};  // logs, keeps the defaults
    CHECK(missing.p_l == 4.f && missing.num_bins_a == 72);
    wave::GroundSegmentation<pcl::PointXYZ> gs{y};
    gs.setKeepGround(true);
    gs.setKeepObstacle(false);
    gs.setKeepOverhanging(false);
    auto copy = gs;
    (void) copy;
    wave::SignalPoint sp{1.0, 2.0, 3, true};
    CHECK(sp.index == 3);
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
