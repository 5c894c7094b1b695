// GroundSegmentation<PointT>::filterBatch against eight filter() calls: a drive of the fixture (the scan after the
// test's car-box removal, moved by step k = 0..7: yaw 0.01 k rad about z, then (0.2 k, 0.05 k, 0) m, in double,
// stored as float) for pcl::PointXYZ and for a 32-byte point type whose extra fields carry the point's index.  The
// outputs must be equal point for point and field for field, with each of the three keep flags flipped once; a null
// entry gives an empty cloud; an empty vector gives none; the filter's own input cloud is left alone.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "wave/matching/ground_segmentation.hpp"
#include "wave/matching/impl/ground_segmentation.hpp"

struct alignas(16) Point32 {  // x, y, z first, then a payload
    float x, y, z, pad;
    float intensity, ring;
    int index, scan;
};
static_assert(sizeof(Point32) == 32, "32-byte point");
template class wave::GroundSegmentation<Point32>;

static int failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failed;                                                   \
        }                                                               \
    } while (0)

static pcl::PointXYZ as(const pcl::PointXYZ &p, int, int, pcl::PointXYZ *) { return p; }
static Point32 as(const pcl::PointXYZ &p, int i, int k, Point32 *) {
    return Point32{p.x, p.y, p.z, 1.f, 0.5f * (float) i, (float) (i % 64), i, k};
}

template <class P>
static bool same(const pcl::PointCloud<P> &a, const pcl::PointCloud<P> &b) {  // every byte of every point
    if (a.points.size() != b.points.size() || a.width != b.width || a.height != b.height || a.is_dense != b.is_dense)
        return false;
    return a.points.empty() || std::memcmp(a.points.data(), b.points.data(), a.points.size() * sizeof(P)) == 0;
}

template <class P>
static size_t run(const std::vector<pcl::PointCloud<pcl::PointXYZ>> &drive, const wave::GroundSegmentationParams &params) {
    using Cloud = pcl::PointCloud<P>;
    std::vector<typename Cloud::ConstPtr> inputs;
    for (size_t k = 0; k < drive.size(); ++k) {
        auto c = boost::make_shared<Cloud>();
        for (size_t i = 0; i < drive[k].points.size(); ++i)
            c->push_back(as(drive[k].points[i], (int) i, (int) k, static_cast<P *>(nullptr)));
        c->is_dense = (k % 2) == 0;  // (carried to the output, whatever it says)
        inputs.push_back(c);
    }
    wave::GroundSegmentation<P> batch{params}, single{params};
    auto own = boost::make_shared<Cloud>(*inputs[3]);
    batch.setInputCloud(own);
    const bool flips[4][3] = {{false, true, true}, {true, true, true}, {false, false, true}, {false, true, false}};
    size_t kept = 0;
    for (const auto &f : flips) {
        batch.setKeepGround(f[0]), single.setKeepGround(f[0]);
        batch.setKeepObstacle(f[1]), single.setKeepObstacle(f[1]);
        batch.setKeepOverhanging(f[2]), single.setKeepOverhanging(f[2]);
        std::vector<Cloud> outputs(2);  // (whatever it held is replaced)
        batch.filterBatch(inputs, outputs);
        CHECK(outputs.size() == inputs.size());
        for (size_t k = 0; k < inputs.size() && k < outputs.size(); ++k) {
            Cloud want;
            single.setInputCloud(inputs[k]);
            single.filter(want);
            CHECK(same(outputs[k], want));
            CHECK(!want.points.empty());
            kept += outputs[k].points.size();
        }
    }
    CHECK(batch.getInputCloud() == own);
    // a null entry: an empty cloud (and a LOG_ERROR), its neighbours as before
    std::vector<typename Cloud::ConstPtr> holed = {inputs[0], typename Cloud::ConstPtr(), inputs[1]};
    std::vector<Cloud> outputs;
    batch.filterBatch(holed, outputs);
    CHECK(outputs.size() == 3);
    if (outputs.size() == 3) {
        Cloud want;
        single.setInputCloud(inputs[0]);
        single.filter(want);
        CHECK(same(outputs[0], want));
        CHECK(outputs[1].points.empty() && outputs[1].width == 0);
        single.setInputCloud(inputs[1]);
        single.filter(want);
        CHECK(same(outputs[2], want));
    }
    // an empty vector
    outputs.resize(5);
    batch.filterBatch(std::vector<typename Cloud::ConstPtr>(), outputs);
    CHECK(outputs.empty());
    // an empty cloud among full ones
    holed[1] = boost::make_shared<Cloud>();
    batch.filterBatch(holed, outputs);
    CHECK(outputs.size() == 3 && outputs[1].points.empty() && !outputs[2].points.empty());
    return kept;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string scan = argv[1], config = argv[2];
    pcl::PointCloud<pcl::PointXYZ> input;
    if (pcl::io::loadPCDFile(scan, input) != 0) return 3;
    pcl::PointCloud<pcl::PointXYZ> fixture;
    for (const auto &p : input.points)
        if (p.x < -3.f || p.x > 3.f || p.y < -1.1f || p.y > 1.1f) fixture.push_back(p);
    std::vector<pcl::PointCloud<pcl::PointXYZ>> drive(8);
    for (int k = 0; k < 8; ++k) {
        const double c = std::cos(0.01 * k), s = std::sin(0.01 * k);
        for (const auto &p : fixture.points) {
            pcl::PointXYZ q;
            q.x = (float) (c * (double) p.x - s * (double) p.y + 0.2 * k);
            q.y = (float) (s * (double) p.x + c * (double) p.y + 0.05 * k);
            q.z = p.z;
            drive[(size_t) k].push_back(q);
        }
    }
    wave::GroundSegmentationParams params{config};
    const size_t a = run<pcl::PointXYZ>(drive, params);
    const size_t b = run<Point32>(drive, params);
    CHECK(a == b && a > 0);
    std::printf("kept %zu %zu\nfailed checks: %d\n", a, b, failed);
    return failed ? 1 : 0;
}
