// wave::ClusterBoxes<pcl::PointXYZ> on a scan: the scan clustered with the YAML fixture's parameters, compute() against
// the bytes the C ABI (wm_cluster_boxes, called here on a context of its own) gives for the same cloud and clusters;
// computeBatch over four clouds against four compute() calls; setters and getters; a copy works on a context of its
// own; a 32-byte point type through the impl header; the PCL-named accessors; a null cloud among a batch, a differing
// number of lists and an index outside the cloud give an empty result.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "wave/matching/cluster_boxes.hpp"
#include "wave/matching/cluster_extraction.hpp"
#include "wave/matching/impl/cluster_boxes.hpp"
#include "wavematch.h"

struct alignas(16) Point32 {  // x, y, z first, then a payload
    float x, y, z, pad;
    float intensity, ring, a, b;
};
static_assert(sizeof(Point32) == 32, "32-byte point");
template class wave::ClusterBoxes<Point32>;

static int failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failed;                                                   \
        }                                                               \
    } while (0)

using Cloud = pcl::PointCloud<pcl::PointXYZ>;
using Clusters = std::vector<pcl::PointIndices>;
using Boxes = std::vector<wave::ClusterBox>;

static std::vector<wm_cluster_box> viaAbi(wm_ctx *ctx, const Cloud &in, const Clusters &clusters) {
    std::vector<int32_t> idx;
    std::vector<uint32_t> off(1, 0);
    for (const auto &c : clusters) {
        idx.insert(idx.end(), c.indices.begin(), c.indices.end());
        off.push_back((uint32_t) idx.size());
    }
    std::vector<wm_cluster_box> out(clusters.size());
    const int rc = wm_cluster_boxes(ctx, in.points.data(), in.size(), sizeof(pcl::PointXYZ), WM_MEM_HOST, idx.data(), idx.size(),
                                    off.data(), clusters.size(), WM_MEM_HOST, out.data(), WM_MEM_HOST, nullptr);
    CHECK(rc == WM_OK);
    return out;
}

template <class A, class B>
static bool sameBytes(const std::vector<A> &a, const std::vector<B> &b) {
    static_assert(sizeof(A) == sizeof(B), "boxes of one size");
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(A)) == 0);
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string scan = argv[1], config = argv[2];
    auto input = boost::make_shared<Cloud>();
    if (pcl::io::loadPCDFile(scan, *input) != 0) return 3;
    wm_ctx *ctx = nullptr;
    if (wm_ctx_create(&ctx, 0) != WM_OK) return 4;

    wave::EuclideanClusterExtraction<pcl::PointXYZ> ec{wave::ClusterExtractionParams{config}};
    ec.setInputCloud(input);
    Clusters clusters;
    ec.extract(clusters);
    CHECK(clusters.size() > 1);

    wave::ClusterBoxes<pcl::PointXYZ> cb;
    cb.setInputCloud(input);
    cb.setClusters(clusters);
    CHECK(cb.getInputCloud() == input && cb.getClusters().size() == clusters.size());
    Boxes got;
    cb.compute(got);
    const std::vector<wm_cluster_box> want = viaAbi(ctx, *input, clusters);
    CHECK(got.size() == clusters.size() && sameBytes(got, want));
    Boxes again;
    cb.compute(again);
    CHECK(sameBytes(again, want));
    std::printf("%zu clusters of %zu points: the largest has %u members, half extents %.3f %.3f %.3f\n", got.size(),
                input->size(), got.empty() ? 0u : got[0].n, got.empty() ? 0.f : got[0].obb_half[0],
                got.empty() ? 0.f : got[0].obb_half[1], got.empty() ? 0.f : got[0].obb_half[2]);

    // the accessors, PCL's names
    for (size_t c = 0; c < got.size(); ++c) {
        const wave::ClusterBox &b = got[c];
        CHECK(b.n == clusters[c].indices.size() && b.flags == 0 && b.hasMoments());
        pcl::PointXYZ lo, hi, pos;
        Eigen::Matrix<float, 3, 3> rot;
        Eigen::Vector3f centre, major, middle, minor;
        float l0, l1, l2;
        CHECK(b.getAABB(lo, hi) && lo.x == b.aabb_min[0] && hi.z == b.aabb_max[2] && lo.y <= hi.y);
        CHECK(b.getOBB(lo, hi, pos, rot) && lo.x == -b.obb_half[0] && hi.y == b.obb_half[1] && pos.z == b.obb_center[2]);
        CHECK(rot(0, 0) == b.axes[0] && rot(1, 0) == b.axes[1] && rot(0, 1) == b.axes[3] && rot(2, 2) == b.axes[8]);
        CHECK(b.getMassCenter(centre) && centre(1) == b.centroid[1]);
        CHECK(b.getEigenValues(l0, l1, l2) && l0 >= l1 && l1 >= l2 && l2 >= 0.f && l0 == b.eigenvalues[0]);
        CHECK(b.getEigenVectors(major, middle, minor) && major(2) == b.axes[2] && minor(0) == b.axes[6]);
        for (int i = 0; i < 3; ++i) CHECK(b.aabb_min[i] <= b.centroid[i] && b.centroid[i] <= b.aabb_max[i]);
    }

    // a copy has its own context, the same cloud and clusters; assignment too
    auto copy = cb;
    Boxes a, b2;
    copy.compute(a);
    cb.compute(b2);
    CHECK(sameBytes(a, want) && sameBytes(b2, want));
    wave::ClusterBoxes<pcl::PointXYZ> assigned;
    assigned = cb;
    assigned.compute(a);
    CHECK(sameBytes(a, want));

    // a 32-byte point type (stride 32): the same bytes
    auto in32 = boost::make_shared<pcl::PointCloud<Point32>>();
    for (const auto &p : input->points) in32->push_back(Point32{p.x, p.y, p.z, 1.f, 7.f, 3.f, -1.f, 2.f});
    wave::ClusterBoxes<Point32> c32;
    c32.setInputCloud(in32);
    c32.setClusters(clusters);
    Boxes b32;
    c32.compute(b32);
    CHECK(sameBytes(b32, want));

    // four clouds in one call: the scan, the scan moved and clustered afresh, a cloud without clusters, an empty cloud
    auto moved = boost::make_shared<Cloud>();
    for (const auto &p : input->points) moved->push_back(pcl::PointXYZ(p.y + 100.f, p.x - 30.f, p.z * 0.5f));
    ec.setInputCloud(moved);
    ec.setClusterTolerance(0.3);
    ec.setMinClusterSize(2);
    ec.setMaxClusterSize(500);
    Clusters moved_clusters;
    ec.extract(moved_clusters);
    CHECK(moved_clusters.size() > 1);
    auto empty = boost::make_shared<Cloud>();
    std::vector<Cloud::ConstPtr> clouds = {input, moved, input, empty};
    std::vector<Clusters> lists = {clusters, moved_clusters, Clusters(), Clusters(2)};  // (two clusters without members)
    std::vector<Boxes> batch;
    cb.computeBatch(clouds, lists, batch);
    CHECK(batch.size() == 4);
    for (size_t k = 0; k < batch.size(); ++k) {
        wave::ClusterBoxes<pcl::PointXYZ> one;
        one.setInputCloud(clouds[k]);
        one.setClusters(lists[k]);
        Boxes single;
        one.compute(single);
        CHECK(single.size() == lists[k].size() && sameBytes(batch[k], single));
    }
    if (batch.size() == 4) {
        CHECK(sameBytes(batch[0], want) && batch[2].empty() && batch[3].size() == 2);
        CHECK(batch[3].size() == 2 && batch[3][0].n == 0 && batch[3][1].flags == wave::ClusterBox::EMPTY && !batch[3][0].hasMoments());
    }
    cb.compute(again);  // the object's own cloud and clusters are as they were
    CHECK(sameBytes(again, want));

    // errors: an empty result
    std::vector<Boxes> none(3);
    clouds[1] = nullptr;
    cb.computeBatch(clouds, lists, none);
    CHECK(none.empty());
    clouds[1] = moved;
    lists.pop_back();
    none.resize(2);
    cb.computeBatch(clouds, lists, none);
    CHECK(none.empty());
    Clusters outside = clusters;
    outside[0].indices[0] = (int) input->size();
    cb.setClusters(outside);
    Boxes nothing(5);
    cb.compute(nothing);
    CHECK(nothing.empty());
    wave::ClusterBoxes<pcl::PointXYZ> no_cloud;
    no_cloud.setClusters(clusters);
    no_cloud.compute(nothing);
    CHECK(nothing.empty());

    wm_ctx_destroy(ctx);
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
