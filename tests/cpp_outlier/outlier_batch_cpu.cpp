// filterBatch links for pcl::PointXYZ (precompiled in libwave_matching.so) and for a 32-byte point type (through the
// impl header).  No device here: an empty queue and a queue without a point return before one is needed, a null cloud
// is logged, and a queue that needs a device logs the failure and gives empty outputs.
#include <cstdio>
#include <vector>

#include "wave/matching/impl/outlier_removal.hpp"
#include "wave/matching/outlier_removal.hpp"

struct alignas(16) Point32 {
    float x, y, z, pad;
    float intensity, ring;
    int index, scan;
};
static_assert(sizeof(Point32) == 32, "32-byte point");
template class wave::OutlierRemoval<Point32>;

static int failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failed;                                                   \
        }                                                               \
    } while (0)

template <class P>
static void none() {
    using Filter = wave::OutlierRemoval<P>;
    wave::OutlierRemovalParams params;
    params.mean_k = 2;
    Filter f{params};
    std::vector<typename Filter::PointCloudConstPtr> clouds;
    std::vector<typename Filter::PointCloud> out(3);
    f.filterBatch(clouds, out);  // nothing to do
    CHECK(out.empty());
    auto empty = boost::make_shared<pcl::PointCloud<P>>();
    clouds.push_back(empty);
    clouds.push_back(typename Filter::PointCloudConstPtr());
    f.filterBatch(clouds, out);  // no point anywhere, a null cloud: logged, empty outputs, no device
    CHECK(out.size() == 2 && out[0].size() == 0 && out[1].size() == 0);
    auto cloud = boost::make_shared<pcl::PointCloud<P>>();
    for (int i = 0; i < 5; ++i) {
        P p{};
        p.x = (float) i;
        cloud->push_back(p);
    }
    clouds.push_back(cloud);
    out.clear();
    f.filterBatch(clouds, out);  // no device to open: logged, empty outputs
    CHECK(out.size() == 3 && out[2].size() == 0);
}

int main() {
    none<pcl::PointXYZ>();
    none<Point32>();
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
