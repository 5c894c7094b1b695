// wave::ISSKeypoint3D<pcl::PointXYZ> on a scan: YAML params, compute() into a second cloud and in place; the keypoint
// cloud must be pcl::copyPointCloud of the indices the C ABI (wm_iss_keypoints, called here on a context of its own)
// returns for the same cloud and parameters, and getKeypointsIndices() those indices.  Also: a copy, a 32-byte point
// type through the impl header keeps its payload, and the refused setters and bad parameters give an empty output.
#include <cstdio>
#include <string>
#include <vector>

#include "wave/matching/impl/iss_keypoints.hpp"
#include "wave/matching/iss_keypoints.hpp"
#include "wavematch.h"

struct alignas(16) Point32 {  // x, y, z first, then a payload
    float x, y, z, pad;
    float intensity, ring, a, b;
};
static_assert(sizeof(Point32) == 32, "32-byte point");
template class wave::ISSKeypoint3D<Point32>;

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

// the C ABI's own keypoints of `in`
static std::vector<int> viaAbi(wm_ctx *ctx, const Cloud &in, const wave::ISSKeypointParams &q) {
    wm_iss_params p;
    wm_iss_default_params(&p);
    p.salient_radius = q.salient_radius, p.non_max_radius = q.non_max_radius, p.gamma_21 = q.gamma_21, p.gamma_32 = q.gamma_32;
    p.min_neighbors = q.min_neighbors;
    std::vector<int> idx(in.size());
    size_t m = 0;
    wm_iss_stats st;
    const int rc = wm_iss_keypoints(ctx, in.points.data(), in.size(), sizeof(pcl::PointXYZ), WM_MEM_HOST, &p, idx.data(),
                                    idx.size(), WM_MEM_HOST, &m, nullptr, nullptr, nullptr, &st);
    CHECK(rc == WM_OK && st.n_keypoints == m && st.n_salient >= m);
    idx.resize(rc == WM_OK ? m : 0);
    return idx;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string scan = argv[1], config = argv[2];
    auto input = boost::make_shared<Cloud>();
    if (pcl::io::loadPCDFile(scan, *input) != 0) return 3;
    wm_ctx *ctx = nullptr;
    if (wm_ctx_create(&ctx, 0) != WM_OK) return 4;

    wave::ISSKeypointParams params{config};
    CHECK(params.salient_radius == 1.0 && params.non_max_radius == 0.5 && params.gamma_21 == 0.975 && params.min_neighbors == 5);
    const std::vector<int> idx = viaAbi(ctx, *input, params);
    Cloud want;
    pcl::copyPointCloud(*input, idx, want);
    CHECK(idx.size() > 10 && idx.size() < input->size() / 4);
    std::printf("keypoints: %zu of %zu\n", idx.size(), input->size());

    wave::ISSKeypoint3D<pcl::PointXYZ> det{params};
    det.setInputCloud(input);
    Cloud second;
    det.compute(second);
    CHECK(same(second, want));
    CHECK(second.height == 1 && second.width == second.size() && second.is_dense == input->is_dense);
    CHECK(det.getKeypointsIndices() && det.getKeypointsIndices()->indices == idx);
    Cloud again;  // a second call detects afresh
    det.compute(again);
    CHECK(same(again, want));

    // the setters give what the file gave; a copy opens its own context; in place
    wave::ISSKeypoint3D<pcl::PointXYZ> by_hand;
    by_hand.setSalientRadius(1.0);
    by_hand.setNonMaxRadius(0.5);
    by_hand.setThreshold21(0.975);
    by_hand.setThreshold32(0.975);
    by_hand.setMinNeighbors(5);
    auto copy = by_hand;
    auto inplace = boost::make_shared<Cloud>(*input);
    copy.setInputCloud(inplace);
    copy.compute(*inplace);
    CHECK(same(*inplace, want));
    CHECK(copy.getKeypointsIndices()->indices == idx && by_hand.getKeypointsIndices()->indices.empty());

    // other parameters give other keypoints, equal to the C ABI's again
    wave::ISSKeypointParams q = params;
    q.salient_radius = 0.6, q.non_max_radius = 0.4, q.min_neighbors = 8;
    wave::ISSKeypoint3D<pcl::PointXYZ> other{q};
    other.setInputCloud(input);
    Cloud third;
    other.compute(third);
    const std::vector<int> idx2 = viaAbi(ctx, *input, q);
    CHECK(other.getKeypointsIndices()->indices == idx2 && idx2 != idx && !idx2.empty());

    // a 32-byte point type (stride 32): the same points, the payload carried along
    auto in32 = boost::make_shared<pcl::PointCloud<Point32>>();
    for (const auto &p : input->points) in32->push_back(Point32{p.x, p.y, p.z, 1.f, 7.f, 3.f, -1.f, 2.f});
    wave::ISSKeypoint3D<Point32> d32{params};
    d32.setInputCloud(in32);
    pcl::PointCloud<Point32> o32;
    d32.compute(o32);
    CHECK(same(o32, want));
    CHECK(!o32.points.empty() && o32.points[0].intensity == 7.f && o32.points[0].b == 2.f);

    // what is not built is refused: a LOG_ERROR and an empty output
    for (int which = 0; which < 2; ++which) {
        wave::ISSKeypoint3D<pcl::PointXYZ> refused{params};
        refused.setInputCloud(input);
        if (which == 0) refused.setBorderRadius(0.3);
        else refused.setNormalRadius(0.3);
        Cloud none = *input;
        refused.compute(none);
        CHECK(none.size() == 0 && refused.getKeypointsIndices()->indices.empty());
        refused.setBorderRadius(0.0);  // (0 is PCL's "no border estimation")
        refused.setNormalRadius(0.0);
        refused.compute(none);
        CHECK(same(none, want));
    }
    // bad parameters: LOG_ERROR and an empty output
    wave::ISSKeypoint3D<pcl::PointXYZ> bad;  // the radii are not set
    bad.setInputCloud(input);
    Cloud none = *input;
    bad.compute(none);
    CHECK(none.size() == 0);

    wm_ctx_destroy(ctx);
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
