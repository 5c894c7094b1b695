// wave::SACSegmentation<PointT>::segmentBatch on a scan cut into four sub-clouds: one batched call must give, cloud for
// cloud, what four segment() calls give -- indices and the coefficients' bits -- for pcl::PointXYZ and a 32-byte point
// type.  Also: a copy works on a context of its own, empty vectors and empty clouds, clouds without a model (two points,
// collinear points), a null cloud (logged, empty outputs), bad parameters.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "wave/matching/impl/sac_segmentation.hpp"
#include "wave/matching/sac_segmentation.hpp"

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

static pcl::PointXYZ make(const pcl::PointXYZ &p, int) { return p; }
static Point32 make32(const pcl::PointXYZ &p, int index) { return Point32{p.x, p.y, p.z, 1.f, 7.f + (float) index, 3.f, 5.f, 9.f}; }

static bool same(const pcl::PointIndices &ia, const pcl::ModelCoefficients &ca, const pcl::PointIndices &ib,
                 const pcl::ModelCoefficients &cb) {
    return ia.indices == ib.indices && ca.values.size() == cb.values.size() &&
           (ca.values.empty() || std::memcmp(ca.values.data(), cb.values.data(), ca.values.size() * sizeof(float)) == 0);
}

template <class P, class Make>
static void run(const pcl::PointCloud<pcl::PointXYZ> &scan, const wave::SACSegmentationParams &params, Make mk, const char *what) {
    using Seg = wave::SACSegmentation<P>;
    using Cloud = pcl::PointCloud<P>;
    // four sub-clouds of different sizes (every 4th point, offset by the cloud's number)
    std::vector<typename Seg::PointCloudConstPtr> clouds;
    for (int s = 0; s < 4; ++s) {
        auto c = boost::make_shared<Cloud>();
        for (size_t i = (size_t) s; i < scan.size() / (size_t) (s + 1); i += 4) c->push_back(mk(scan.points[i], (int) i));
        clouds.push_back(c);
    }
    for (int optimize = 0; optimize < 2; ++optimize) {
        Seg seg{params};
        seg.setOptimizeCoefficients(optimize != 0);
        std::vector<pcl::PointIndices> want_i(4), got_i(1);
        std::vector<pcl::ModelCoefficients> want_c(4), got_c(7);
        size_t in = 0, planes = 0;
        for (int s = 0; s < 4; ++s) {
            seg.setInputCloud(clouds[s]);
            seg.segment(want_i[s], want_c[s]);
            CHECK(want_c[s].values.size() == 4 && !want_i[s].indices.empty());
            planes += want_i[s].indices.size();
            in += clouds[s]->size();
        }
        seg.segmentBatch(clouds, got_i, got_c);
        CHECK(got_i.size() == 4 && got_c.size() == 4);
        for (int s = 0; s < 4 && got_i.size() == 4 && got_c.size() == 4; ++s) CHECK(same(got_i[s], got_c[s], want_i[s], want_c[s]));
        auto copy = seg;  // (the copy opens its own context)
        std::vector<pcl::PointIndices> again_i;
        std::vector<pcl::ModelCoefficients> again_c;
        copy.segmentBatch(clouds, again_i, again_c);
        CHECK(again_i.size() == 4 && again_c.size() == 4);
        for (int s = 0; s < 4 && again_i.size() == 4 && again_c.size() == 4; ++s)
            CHECK(same(again_i[s], again_c[s], want_i[s], want_c[s]));
        std::printf("%s optimize %d: %zu plane points of %zu in four clouds\n", what, optimize, planes, in);
    }

    // empty vectors, empty clouds, a null cloud, clouds without a model
    Seg seg{params};
    std::vector<typename Seg::PointCloudConstPtr> mixed;
    std::vector<pcl::PointIndices> out_i(2);
    std::vector<pcl::ModelCoefficients> out_c(2);
    seg.segmentBatch(mixed, out_i, out_c);
    CHECK(out_i.empty() && out_c.empty());
    auto two = boost::make_shared<Cloud>();
    for (int i = 0; i < 2; ++i) two->push_back(mk(scan.points[i], i));
    auto line = boost::make_shared<Cloud>();
    for (int i = 0; i < 40; ++i) line->push_back(mk(pcl::PointXYZ((float) i, 2.f * (float) i, 0.5f * (float) i), i));
    mixed.push_back(clouds[2]);
    mixed.push_back(typename Seg::PointCloudConstPtr());
    mixed.push_back(boost::make_shared<Cloud>());
    mixed.push_back(two);
    mixed.push_back(line);
    mixed.push_back(clouds[3]);
    seg.segmentBatch(mixed, out_i, out_c);
    CHECK(out_i.size() == 6 && out_c.size() == 6);
    if (out_i.size() == 6 && out_c.size() == 6) {
        pcl::PointIndices i2, i3;
        pcl::ModelCoefficients c2, c3;
        seg.setInputCloud(clouds[2]);
        seg.segment(i2, c2);
        seg.setInputCloud(clouds[3]);
        seg.segment(i3, c3);
        CHECK(same(out_i[0], out_c[0], i2, c2) && same(out_i[5], out_c[5], i3, c3));
        for (int k = 1; k < 5; ++k) CHECK(out_i[k].indices.empty() && out_c[k].values.empty());
    }

    // bad parameters: LOG_ERROR and empty outputs
    wave::SACSegmentationParams bad = params;
    bad.distance_threshold = 0;
    Seg sb{bad};
    std::vector<pcl::PointIndices> none_i(1);
    std::vector<pcl::ModelCoefficients> none_c(1);
    sb.segmentBatch(clouds, none_i, none_c);
    CHECK(none_i.size() == 4 && none_c.size() == 4);
    for (const auto &i : none_i) CHECK(i.indices.empty());
    for (const auto &c : none_c) CHECK(c.values.empty());
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string scan_path = argv[1], config = argv[2];
    pcl::PointCloud<pcl::PointXYZ> scan;
    if (pcl::io::loadPCDFile(scan_path, scan) != 0) return 3;
    wave::SACSegmentationParams params{config};
    CHECK(params.distance_threshold == 0.2 && params.max_iterations == 100 && params.seed == 3);
    run<pcl::PointXYZ>(scan, params, make, "PointXYZ");
    run<Point32>(scan, params, make32, "Point32");
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
