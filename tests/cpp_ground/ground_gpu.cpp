// The reference's how_to_use flow (wave_matching/tests/ground_segmentation_test.cpp) without the viewer: load the
// PCD, remove the car's box by hand (the test's pcl::ConditionalRemoval), YAML params, filter() three times with
// the three keep settings on one object.  The three clouds are written out (float x y z per point) for
// tests/test_ground_cpp.py to compare with the checker.  Also: repeated filter() calls do not accumulate, filter()
// in place, and a custom 32-byte point type that starts with x, y, z (the impl header instantiates it).
#include <cstdio>
#include <string>

#include "wave/matching/ground_segmentation.hpp"
#include "wave/matching/impl/ground_segmentation.hpp"

struct alignas(16) Point32 {  // x, y, z first, then a payload
    float x, y, z, pad;
    float intensity, ring, a, b;
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

template <class P>
static void dump(const pcl::PointCloud<P> &c, const std::string &path) {
    FILE *f = std::fopen(path.c_str(), "wb");
    for (const auto &p : c.points) {
        const float v[3] = {p.x, p.y, p.z};
        std::fwrite(v, sizeof(float), 3, f);
    }
    std::fclose(f);
}

template <class P>
static bool same(const pcl::PointCloud<P> &a, const pcl::PointCloud<pcl::PointXYZ> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a.points[i].x != b.points[i].x || a.points[i].y != b.points[i].y || a.points[i].z != b.points[i].z) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const std::string scan = argv[1], config = argv[2], out = argv[3];
    auto input = boost::make_shared<pcl::PointCloud<pcl::PointXYZ>>();
    if (pcl::io::loadPCDFile(scan, *input) != 0) return 3;
    // the test's car-box removal: keep (x < -3 or x > 3) or (y < -1.1 or y > 1.1), compared as floats
    pcl::PointCloud<pcl::PointXYZ> kept;
    for (const auto &p : input->points)
        if (p.x < -3.f || p.x > 3.f || p.y < -1.1f || p.y > 1.1f) kept.push_back(p);
    kept.is_dense = input->is_dense;
    *input = kept;

    using Cloud = pcl::PointCloud<pcl::PointXYZ>;
    auto cl_ground = boost::make_shared<Cloud>(), cl_obstacle = boost::make_shared<Cloud>(), cl_overhang = boost::make_shared<Cloud>();
    wave::GroundSegmentationParams params{config};
    wave::GroundSegmentation<pcl::PointXYZ> gs{params};
    gs.setInputCloud(input);

    gs.setKeepGround(true);
    gs.setKeepObstacle(false);
    gs.setKeepOverhanging(false);
    gs.filter(*cl_ground);

    gs.setKeepGround(false);
    gs.setKeepObstacle(true);
    gs.filter(*cl_obstacle);

    gs.setKeepObstacle(false);
    gs.setKeepOverhanging(true);
    gs.filter(*cl_overhang);

    dump(*cl_ground, out + "/ground.bin");
    dump(*cl_obstacle, out + "/obstacle.bin");
    dump(*cl_overhang, out + "/overhanging.bin");
    CHECK(cl_ground->size() > 0 && cl_obstacle->size() > 0 && cl_overhang->size() > 0);
    CHECK(cl_ground->height == 1 && cl_ground->width == cl_ground->size());

    // repeated calls classify afresh (the reference's index vectors would grow)
    pcl::PointCloud<pcl::PointXYZ> again;
    gs.filter(again);
    CHECK(same(again, *cl_overhang));

    // in place: filter(*input_)
    auto inplace = boost::make_shared<Cloud>(*input);
    wave::GroundSegmentation<pcl::PointXYZ> gs2{params};
    gs2.setInputCloud(inplace);
    gs2.setKeepGround(true);
    gs2.setKeepObstacle(false);
    gs2.setKeepOverhanging(false);
    gs2.filter(*inplace);
    CHECK(same(*inplace, *cl_ground));

    // a 32-byte point type (stride 32)
    auto in32 = boost::make_shared<pcl::PointCloud<Point32>>();
    for (const auto &p : input->points) in32->push_back(Point32{p.x, p.y, p.z, 1.f, 7.f, 3.f, -1.f, 2.f});
    wave::GroundSegmentation<Point32> gs32{params};
    gs32.setInputCloud(in32);
    pcl::PointCloud<Point32> o32;
    gs32.filter(o32);  // default keep: obstacle + overhanging
    pcl::PointCloud<pcl::PointXYZ> both;
    gs.setKeepObstacle(true);  // (ground off, obstacle and overhanging on)
    gs.filter(both);
    CHECK(same(o32, both));
    CHECK(!o32.points.empty() && o32.points[0].intensity == 7.f && o32.points[0].b == 2.f);

    // bad parameters: LOG_ERROR and an empty output
    wave::GroundSegmentationParams bad = params;
    bad.num_bins_a = 0;
    wave::GroundSegmentation<pcl::PointXYZ> gs_bad{bad};
    gs_bad.setInputCloud(input);
    pcl::PointCloud<pcl::PointXYZ> none;
    gs_bad.filter(none);
    CHECK(none.size() == 0);

    std::printf("sizes %zu %zu %zu\nfailed checks: %d\n", cl_ground->size(), cl_obstacle->size(), cl_overhang->size(), failed);
    return failed ? 1 : 0;
}
