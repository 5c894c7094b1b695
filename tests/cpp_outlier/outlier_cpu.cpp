// The C++ drop-in away from any device: the defaults are PCL's, the YAML constructor reads its six keys, a missing
// file keeps the defaults, and an OutlierRemoval is constructed, configured and copied without opening a device.
#include <cstdio>

#include "wave/matching/outlier_removal.hpp"

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
    wave::OutlierRemovalParams d{};
    CHECK(d.method == wave::OutlierRemovalParams::Statistical && d.mean_k == 1 && d.stddev_mult == 0);
    CHECK(d.radius == 0 && d.min_neighbors == 1 && d.negative == 0);
    wave::OutlierRemovalParams y{std::string(argv[1])};
    CHECK(y.method == 0 && y.mean_k == 8 && y.stddev_mult == 1.0 && y.radius == 0.5 && y.min_neighbors == 5);
    CHECK(y.negative == 0);
    wave::OutlierRemovalParams missing{std::string("/nonexistent/outlier.yaml")};  // logs, keeps the defaults
    CHECK(missing.mean_k == 1 && missing.min_neighbors == 1);
    wave::OutlierRemoval<pcl::PointXYZ> f{y};
    CHECK(!f.getNegative());
    f.setNegative(true);
    auto copy = f;
    CHECK(copy.getNegative());
    wave::OutlierRemoval<pcl::PointXYZ> other{d};
    other = f;
    CHECK(other.getNegative());
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
