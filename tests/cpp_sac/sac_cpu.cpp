// The C++ drop-in away from any device: the defaults are PCL's, the YAML constructor reads its keys, a missing file
// keeps the defaults, and a SACSegmentation is constructed, configured and copied without opening a device; segment()
// without an input cloud, with an unbuilt model or method returns nothing; the C ABI's argument errors and n < 3 come
// back without a device.
#include <cstdio>

#include "wave/matching/sac_segmentation.hpp"
#include "wavematch.h"

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
    wave::SACSegmentationParams d{};
    CHECK(d.model_type == pcl::SACMODEL_PLANE && d.method_type == pcl::SAC_RANSAC && d.distance_threshold == 0);
    CHECK(d.max_iterations == 50 && d.probability == 0.99 && d.optimize_coefficients && d.seed == 0 && d.eps_angle == 0);
    wm_sac_params c;
    wm_sac_default_params(&c);
    CHECK(c.model == WM_SAC_PLANE && c.distance_threshold == d.distance_threshold && c.max_iterations == d.max_iterations);
    CHECK(c.probability == d.probability && c.optimize_coefficients == 1 && c.seed == 0);
    wave::SACSegmentationParams y{std::string(argv[1])};
    CHECK(y.model_type == 0 && y.distance_threshold == 0.2 && y.max_iterations == 100 && y.probability == 0.99);
    CHECK(y.optimize_coefficients && y.axis[0] == 0 && y.axis[1] == 0 && y.axis[2] == 1 && y.eps_angle == 0.1 && y.seed == 3);
    wave::SACSegmentationParams missing{std::string("/nonexistent/sac.yaml")};  // logs, keeps the defaults
    CHECK(missing.distance_threshold == 0 && missing.max_iterations == 50 && missing.seed == 0);

    wave::SACSegmentation<pcl::PointXYZ> plain;
    CHECK(plain.getDistanceThreshold() == 0 && plain.getMaxIterations() == 50 && plain.getProbability() == 0.99);
    CHECK(plain.getOptimizeCoefficients() && plain.getModelType() == pcl::SACMODEL_PLANE && plain.getSeed() == 0);
    wave::SACSegmentation<pcl::PointXYZ> seg{y};
    CHECK(seg.getDistanceThreshold() == 0.2 && seg.getMaxIterations() == 100 && seg.getSeed() == 3);
    seg.setDistanceThreshold(0.25);
    seg.setModelType(pcl::SACMODEL_PARALLEL_PLANE);
    seg.setAxis(1.0, 0.0, 0.0);
    seg.setEpsAngle(0.3);
    auto copy = seg;
    CHECK(copy.getDistanceThreshold() == 0.25 && copy.getModelType() == pcl::SACMODEL_PARALLEL_PLANE);
    CHECK(copy.getAxis()[0] == 1.0 && copy.getEpsAngle() == 0.3);
    plain = seg;
    CHECK(plain.getDistanceThreshold() == 0.25 && plain.getEpsAngle() == 0.3 && !plain.getInputCloud());
    pcl::PointIndices inliers;
    pcl::ModelCoefficients coef;
    inliers.indices.assign(2, 5);
    coef.values.assign(4, 1.f);
    plain.segment(inliers, coef);  // no input cloud: nothing, and no device
    CHECK(inliers.indices.empty() && coef.values.empty());
    auto cloud = boost::make_shared<pcl::PointCloud<pcl::PointXYZ>>();
    for (int k = 0; k < 10; ++k) cloud->push_back(pcl::PointXYZ{(float) k, (float) (k * k), 0.f});
    plain.setInputCloud(cloud);
    plain.setModelType(5);  // (pcl::SACMODEL_CYLINDER): refused before a device is opened
    coef.values.assign(4, 1.f);
    plain.segment(inliers, coef);
    CHECK(inliers.indices.empty() && coef.values.empty());
    plain.setModelType(pcl::SACMODEL_PLANE);
    plain.setMethodType(1);  // (pcl::SAC_LMEDS)
    plain.segment(inliers, coef);
    CHECK(inliers.indices.empty() && coef.values.empty());

    // the C ABI: argument errors and n < 3 without a device (the context pointer is never followed)
    wm_ctx *fake = reinterpret_cast<wm_ctx *>(16);
    float pts[12] = {0}, out[4];
    int32_t idx[4];
    size_t m = 7;
    c.distance_threshold = 0.1;
    CHECK(wm_sac_segment(fake, pts, 2, 12, WM_MEM_HOST, &c, out, idx, 4, WM_MEM_HOST, &m, nullptr, nullptr) == WM_NOT_CONVERGED);
    CHECK(m == 0);
    CHECK(wm_sac_segment(fake, pts, 4, 12, WM_MEM_HOST, &c, nullptr, idx, 4, WM_MEM_HOST, &m, nullptr, nullptr) == WM_ERR_ARG);
    c.distance_threshold = 0;
    CHECK(wm_sac_segment(fake, pts, 4, 12, WM_MEM_HOST, &c, out, idx, 4, WM_MEM_HOST, &m, nullptr, nullptr) == WM_ERR_ARG);
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
