// wave::OutlierRemoval<PointT>::filterBatch on a scan cut into four sub-clouds: one batched call must give, cloud for
// cloud, what four filter() calls give -- for pcl::PointXYZ and a 32-byte point type (whose payload is carried along),
// for both filters.  Also: a copy works on a context of its own, empty vectors and empty clouds, a cloud with too few
// points for the statistical filter, a null cloud (logged, an empty output), bad parameters.
#include <cstdio>
#include <string>
#include <vector>

#include "wave/matching/impl/outlier_removal.hpp"
#include "wave/matching/outlier_removal.hpp"

struct alignas(16) Point32 {  // x, y, z first, then a payload
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

static pcl::PointXYZ make(const pcl::PointXYZ &p, int, int) { return p; }
static Point32 make32(const pcl::PointXYZ &p, int index, int scan) {
    return Point32{p.x, p.y, p.z, 1.f, 7.f + (float) index, 3.f, index, scan};
}
static bool payload(const pcl::PointXYZ &, const pcl::PointXYZ &) { return true; }
static bool payload(const Point32 &a, const Point32 &b) {
    return a.intensity == b.intensity && a.index == b.index && a.scan == b.scan;
}

template <class P>
static bool same(const pcl::PointCloud<P> &a, const pcl::PointCloud<P> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a.points[i].x != b.points[i].x || a.points[i].y != b.points[i].y || a.points[i].z != b.points[i].z ||
            !payload(a.points[i], b.points[i]))
            return false;
    return true;
}

template <class P, class Make>
static void run(const pcl::PointCloud<pcl::PointXYZ> &scan, const wave::OutlierRemovalParams &params, Make mk, const char *what) {
    using Filter = wave::OutlierRemoval<P>;
    using Cloud = pcl::PointCloud<P>;
    // four sub-clouds of different sizes (every 4th point, offset by the scan's number)
    std::vector<typename Filter::PointCloudConstPtr> clouds;
    for (int s = 0; s < 4; ++s) {
        auto c = boost::make_shared<Cloud>();
        for (size_t i = (size_t) s; i < scan.size() / (size_t) (s + 1); i += 4) c->push_back(mk(scan.points[i], (int) i, s));
        clouds.push_back(c);
    }
    for (int method = 0; method < 2; ++method)
        for (int negative = 0; negative < 2; ++negative) {
            wave::OutlierRemovalParams q = params;
            q.method = method;
            Filter f{q};
            f.setNegative(negative != 0);
            std::vector<Cloud> want(4);
            size_t kept = 0, in = 0;
            for (int s = 0; s < 4; ++s) {
                f.setInputCloud(clouds[s]);
                f.filter(want[s]);
                kept += want[s].size();
                in += clouds[s]->size();
            }
            CHECK(kept > 0 && kept < in);
            std::vector<Cloud> got(1);
            f.filterBatch(clouds, got);
            CHECK(got.size() == 4);
            for (int s = 0; s < 4 && got.size() == 4; ++s) {
                CHECK(same(got[s], want[s]));
                CHECK(got[s].height == 1 && got[s].width == got[s].size() && got[s].is_dense == clouds[s]->is_dense);
            }
            auto g = f;  // (the copy opens its own context)
            std::vector<Cloud> again;
            g.filterBatch(clouds, again);
            CHECK(again.size() == 4);
            for (int s = 0; s < 4 && again.size() == 4; ++s) CHECK(same(again[s], want[s]));
            std::printf("%s method %d negative %d: kept %zu of %zu in four clouds\n", what, method, negative, kept, in);
        }

    // empty vectors, empty clouds, a null cloud, a cloud with too few points for mean_k
    wave::OutlierRemovalParams q = params;
    q.method = 0;
    Filter f{q};
    std::vector<typename Filter::PointCloudConstPtr> mixed;
    std::vector<Cloud> out(2);
    f.filterBatch(mixed, out);
    CHECK(out.empty());
    auto few = boost::make_shared<Cloud>();
    for (int i = 0; i < 3; ++i) few->push_back(mk(scan.points[i], i, 9));
    mixed.push_back(clouds[2]);
    mixed.push_back(typename Filter::PointCloudConstPtr());
    mixed.push_back(boost::make_shared<Cloud>());
    mixed.push_back(few);
    mixed.push_back(clouds[3]);
    f.filterBatch(mixed, out);
    CHECK(out.size() == 5);
    if (out.size() == 5) {
        Cloud w2, w3;
        f.setInputCloud(clouds[2]);
        f.filter(w2);
        f.setInputCloud(clouds[3]);
        f.filter(w3);
        CHECK(same(out[0], w2) && same(out[4], w3));
        CHECK(out[1].size() == 0 && out[2].size() == 0 && out[3].size() == 0);
    }

    // bad parameters: LOG_ERROR and empty outputs
    wave::OutlierRemovalParams bad = params;
    bad.method = 0;
    bad.mean_k = 50;
    Filter fb{bad};
    std::vector<Cloud> none(1);
    fb.filterBatch(clouds, none);
    CHECK(none.size() == 4);
    for (const auto &c : none) CHECK(c.size() == 0);
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string scan_path = argv[1], config = argv[2];
    pcl::PointCloud<pcl::PointXYZ> scan;
    if (pcl::io::loadPCDFile(scan_path, scan) != 0) return 3;
    wave::OutlierRemovalParams params{config};
    CHECK(params.mean_k == 8 && params.stddev_mult == 1.0);
    run<pcl::PointXYZ>(scan, params, make, "PointXYZ");
    run<Point32>(scan, params, make32, "Point32");
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
