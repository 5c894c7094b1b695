// filterBatch links for pcl::PointXYZ (precompiled in libwave_matching.so) and for a 32-byte point type (through the
// impl header); nothing here opens a device: an empty queue returns before one is needed.
#include <cstdio>
#include <vector>

#include "wave/matching/ground_segmentation.hpp"
#include "wave/matching/impl/ground_segmentation.hpp"

struct alignas(16) Point32 {
    float x, y, z, pad;
    float intensity, ring;
    int index, scan;
};
static_assert(sizeof(Point32) == 32, "32-byte point");
template class wave::GroundSegmentation<Point32>;

template <class P>
static int none() {
    wave::GroundSegmentationParams params;
    wave::GroundSegmentation<P> gs{params};
    std::vector<typename wave::GroundSegmentation<P>::PointCloudConstPtr> inputs;
    std::vector<pcl::PointCloud<P>> outputs(3);
    gs.filterBatch(inputs, outputs);
    return outputs.empty() ? 0 : 1;
}

int main() {
    const int failed = none<pcl::PointXYZ>() + none<Point32>();
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
