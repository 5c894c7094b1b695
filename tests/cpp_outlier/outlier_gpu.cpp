// wave::OutlierRemoval<pcl::PointXYZ> on a scan: YAML params, filter() into a second cloud and in place, both
// filters and both settings of setNegative.  Every kept cloud must be pcl::copyPointCloud of the indices the C ABI
// (wm_outlier_filter, called here on a context of its own) keeps for the same cloud and parameters.  Also: a 32-byte
// point type through the impl header keeps its payload, and bad parameters give an empty output.
#include <cstdio>
#include <string>
#include <vector>

#include "wave/matching/impl/outlier_removal.hpp"
#include "wave/matching/outlier_removal.hpp"
#include "wavematch.h"

struct alignas(16) Point32 {  // x, y, z first, then a payload
    float x, y, z, pad;
    float intensity, ring, a, b;
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

using Cloud = pcl::PointCloud<pcl::PointXYZ>;

template <class P>
static bool same(const pcl::PointCloud<P> &a, const Cloud &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a.points[i].x != b.points[i].x || a.points[i].y != b.points[i].y || a.points[i].z != b.points[i].z) return false;
    return true;
}

// the C ABI's own kept points of `in`
static Cloud viaAbi(wm_ctx *ctx, const Cloud &in, const wave::OutlierRemovalParams &q) {
    wm_outlier_params p;
    wm_outlier_default_params(&p);
    p.method = q.method, p.mean_k = q.mean_k, p.stddev_mult = q.stddev_mult, p.radius = q.radius;
    p.min_neighbors = q.min_neighbors, p.negative = q.negative;
    std::vector<int> idx(in.size());
    size_t m = 0;
    const int rc = wm_outlier_filter(ctx, in.points.data(), in.size(), sizeof(pcl::PointXYZ), WM_MEM_HOST, &p, idx.data(),
                                     idx.size(), WM_MEM_HOST, &m, nullptr, nullptr, nullptr, nullptr);
    CHECK(rc == WM_OK);
    idx.resize(rc == WM_OK ? m : 0);
    Cloud out;
    pcl::copyPointCloud(in, idx, out);
    return out;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string scan = argv[1], config = argv[2];
    auto input = boost::make_shared<Cloud>();
    if (pcl::io::loadPCDFile(scan, *input) != 0) return 3;
    wm_ctx *ctx = nullptr;
    if (wm_ctx_create(&ctx, 0) != WM_OK) return 4;

    wave::OutlierRemovalParams params{config};
    CHECK(params.mean_k == 8 && params.stddev_mult == 1.0);
    for (int method = 0; method < 2; ++method)
        for (int negative = 0; negative < 2; ++negative) {
            wave::OutlierRemovalParams q = params;
            q.method = method;
            wave::OutlierRemoval<pcl::PointXYZ> f{q};
            f.setNegative(negative != 0);
            q.negative = negative;
            const Cloud want = viaAbi(ctx, *input, q);
            f.setInputCloud(input);
            Cloud second;
            f.filter(second);
            CHECK(same(second, want));
            CHECK(second.height == 1 && second.width == second.size() && second.is_dense == input->is_dense);
            CHECK(want.size() > 0 && want.size() < input->size());
            Cloud again;  // a second call filters afresh
            f.filter(again);
            CHECK(same(again, want));
            auto inplace = boost::make_shared<Cloud>(*input);
            auto g = f;  // (the copy opens its own context)
            g.setInputCloud(inplace);
            g.filter(*inplace);
            CHECK(same(*inplace, want));
            std::printf("method %d negative %d: kept %zu of %zu\n", method, negative, want.size(), input->size());
        }

    // a 32-byte point type (stride 32): the same points, the payload carried along
    auto in32 = boost::make_shared<pcl::PointCloud<Point32>>();
    for (const auto &p : input->points) in32->push_back(Point32{p.x, p.y, p.z, 1.f, 7.f, 3.f, -1.f, 2.f});
    wave::OutlierRemoval<Point32> f32{params};
    f32.setInputCloud(in32);
    pcl::PointCloud<Point32> o32;
    f32.filter(o32);
    CHECK(same(o32, viaAbi(ctx, *input, params)));
    CHECK(!o32.points.empty() && o32.points[0].intensity == 7.f && o32.points[0].b == 2.f);

    // bad parameters: LOG_ERROR and an empty output
    wave::OutlierRemovalParams bad = params;
    bad.mean_k = 50;  // PCL's tutorial value: beyond the list limit
    wave::OutlierRemoval<pcl::PointXYZ> fb{bad};
    fb.setInputCloud(input);
    Cloud none;
    fb.filter(none);
    CHECK(none.size() == 0);

    wm_ctx_destroy(ctx);
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
