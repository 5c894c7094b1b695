// wave::SACSegmentation<pcl::PointXYZ> on a scan: YAML params, segment() against what the C ABI (wm_sac_segment, called
// here on a context of its own) gives for the same cloud and parameters; setters and getters; a copy works on a
// context of its own; a 32-byte point type through the impl header; bad parameters and a cloud without a plane give
// empty outputs.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "wave/matching/impl/sac_segmentation.hpp"
#include "wave/matching/sac_segmentation.hpp"
#include "wavematch.h"

struct alignas(16) Point32 {  // x, y, z first, then a payload
    float x, y, z, pad;
    float intensity, ring, a, b;
};
static_assert(sizeof(Point32) == 32, "32-byte point");
template class wave::SACSegmentation<Point32>;

static int failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failed;                                                   \
        }                                                               \
    } while (0)

using Cloud = pcl::PointCloud<pcl::PointXYZ>;

struct Plane {
    std::vector<int> indices;
    std::vector<float> values;
    int rc = 0;
};

static Plane viaAbi(wm_ctx *ctx, const Cloud &in, const wave::SACSegmentationParams &q, int model) {
    wm_sac_params p;
    wm_sac_default_params(&p);
    p.model = model;
    p.distance_threshold = q.distance_threshold;
    p.max_iterations = q.max_iterations;
    p.probability = q.probability;
    p.optimize_coefficients = q.optimize_coefficients ? 1 : 0;
    for (int k = 0; k < 3; ++k) p.axis[k] = q.axis[k];
    p.eps_angle = q.eps_angle;
    p.seed = q.seed;
    std::vector<int32_t> idx(in.size());
    float coef[4];
    size_t m = 0;
    Plane out;
    out.rc = wm_sac_segment(ctx, in.points.data(), in.size(), sizeof(pcl::PointXYZ), WM_MEM_HOST, &p, coef, idx.data(),
                            idx.size(), WM_MEM_HOST, &m, nullptr, nullptr);
    if (out.rc == WM_OK) {
        out.indices.assign(idx.begin(), idx.begin() + m);
        out.values.assign(coef, coef + 4);
    }
    return out;
}

static bool same(const pcl::PointIndices &i, const pcl::ModelCoefficients &c, const Plane &want) {
    return i.indices == want.indices && c.values.size() == want.values.size() &&
           (c.values.empty() || std::memcmp(c.values.data(), want.values.data(), 4 * sizeof(float)) == 0);
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string scan = argv[1], config = argv[2];
    auto input = boost::make_shared<Cloud>();
    if (pcl::io::loadPCDFile(scan, *input) != 0) return 3;
    wm_ctx *ctx = nullptr;
    if (wm_ctx_create(&ctx, 0) != WM_OK) return 4;

    wave::SACSegmentationParams params{config};
    CHECK(params.distance_threshold == 0.2 && params.max_iterations == 100 && params.seed == 3 && params.optimize_coefficients);
    wave::SACSegmentation<pcl::PointXYZ> seg{params};
    seg.setInputCloud(input);
    CHECK(seg.getInputCloud() == input);
    pcl::PointIndices inliers;
    pcl::ModelCoefficients coef;
    seg.segment(inliers, coef);
    const Plane want = viaAbi(ctx, *input, params, WM_SAC_PLANE);
    CHECK(want.rc == WM_OK && same(inliers, coef, want));
    CHECK(coef.values.size() == 4 && inliers.indices.size() > input->size() / 10);
    if (coef.values.size() == 4) {
        const double a = coef.values[0], b = coef.values[1], c = coef.values[2], d = coef.values[3];
        CHECK(std::fabs(std::sqrt(a * a + b * b + c * c) - 1.0) < 1e-6);
        for (size_t j = 0; j < inliers.indices.size(); ++j) {
            const auto &p = input->points[inliers.indices[j]];
            if (j) CHECK(inliers.indices[j] > inliers.indices[j - 1]);
            CHECK(std::fabs(a * p.x + b * p.y + c * p.z + d) < 0.2 * (1 + 1e-5) + 1e-5);
        }
        std::printf("threshold 0.2: plane %.6f %.6f %.6f %.6f with %zu of %zu points\n", a, b, c, d, inliers.indices.size(),
                    input->size());
    }
    pcl::PointIndices again_i;  // a second call segments afresh, to the same bytes
    pcl::ModelCoefficients again_c;
    seg.segment(again_i, again_c);
    CHECK(same(again_i, again_c, want));

    // setters and getters; a copy has its own context and the same settings
    seg.setDistanceThreshold(0.05);
    seg.setMaxIterations(200);
    seg.setProbability(0.999);
    seg.setOptimizeCoefficients(false);
    seg.setSeed(11);
    seg.setModelType(pcl::SACMODEL_PERPENDICULAR_PLANE);
    seg.setAxis(0.0, 0.0, 2.0);
    seg.setEpsAngle(0.2);
    seg.setMethodType(pcl::SAC_RANSAC);
    CHECK(seg.getDistanceThreshold() == 0.05 && seg.getMaxIterations() == 200 && seg.getProbability() == 0.999);
    CHECK(!seg.getOptimizeCoefficients() && seg.getSeed() == 11 && seg.getModelType() == pcl::SACMODEL_PERPENDICULAR_PLANE);
    CHECK(seg.getAxis()[2] == 2.0 && seg.getEpsAngle() == 0.2 && seg.getMethodType() == pcl::SAC_RANSAC);
    auto copy = seg;
    pcl::PointIndices ia, ib;
    pcl::ModelCoefficients ca, cb;
    copy.segment(ia, ca);
    seg.segment(ib, cb);
    wave::SACSegmentationParams q2 = params;
    q2.distance_threshold = 0.05, q2.max_iterations = 200, q2.probability = 0.999, q2.optimize_coefficients = false, q2.seed = 11;
    q2.axis[0] = 0, q2.axis[1] = 0, q2.axis[2] = 2.0, q2.eps_angle = 0.2;
    const Plane want2 = viaAbi(ctx, *input, q2, WM_SAC_PERPENDICULAR_PLANE);
    CHECK(want2.rc == WM_OK && same(ia, ca, want2) && same(ib, cb, want2) && !same(ia, ca, want));
    if (ca.values.size() == 4) CHECK(std::fabs(ca.values[2]) >= std::cos(0.2) - 1e-6);
    std::printf("perpendicular to z, threshold 0.05: %zu points\n", ia.indices.size());

    // a 32-byte point type (stride 32): the same plane
    auto in32 = boost::make_shared<pcl::PointCloud<Point32>>();
    for (const auto &p : input->points) in32->push_back(Point32{p.x, p.y, p.z, 1.f, 7.f, 3.f, -1.f, 2.f});
    wave::SACSegmentation<Point32> s32{params};
    s32.setInputCloud(in32);
    pcl::PointIndices i32;
    pcl::ModelCoefficients c32;
    s32.segment(i32, c32);
    CHECK(same(i32, c32, want));

    // bad parameters, an unbuilt model or method, a cloud without a plane: LOG_ERROR and both outputs empty
    wave::SACSegmentation<pcl::PointXYZ> bad;  // PCL's default threshold 0
    bad.setInputCloud(input);
    pcl::PointIndices none_i;
    pcl::ModelCoefficients none_c;
    none_i.indices.assign(3, 1);
    none_c.values.assign(4, 1.f);
    bad.segment(none_i, none_c);
    CHECK(none_i.indices.empty() && none_c.values.empty());
    bad.setDistanceThreshold(0.2);
    bad.setModelType(4);  // (pcl::SACMODEL_SPHERE)
    none_c.values.assign(4, 1.f);
    bad.segment(none_i, none_c);
    CHECK(none_i.indices.empty() && none_c.values.empty());
    bad.setModelType(pcl::SACMODEL_PLANE);
    bad.setMethodType(2);  // (pcl::SAC_MSAC)
    bad.segment(none_i, none_c);
    CHECK(none_i.indices.empty() && none_c.values.empty());
    bad.setMethodType(pcl::SAC_RANSAC);
    auto line = boost::make_shared<Cloud>();
    for (int k = 0; k < 100; ++k) line->push_back(pcl::PointXYZ{(float) k, 2.f, 3.f});
    bad.setInputCloud(line);
    none_i.indices.assign(3, 1);
    bad.segment(none_i, none_c);  // every sample is collinear
    CHECK(none_i.indices.empty() && none_c.values.empty());
    bad.setInputCloud(input);
    bad.segment(none_i, none_c);
    CHECK(!none_i.indices.empty() && none_c.values.size() == 4);

    wm_ctx_destroy(ctx);
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
