// wave::CorrespondenceRejectorSampleConsensus<pcl::PointXYZ> on the scan fixture with the YAML fixture's parameters:
// the pipeline FPFHEstimation -> matchFeatures(reciprocal) -> the rejector on the scan and a copy of it moved by a known
// pose; the remaining correspondences and the transformation against the bytes the C ABI (wm_corr_ransac, called here
// on a context of its own) gives for the same correspondences; a copy works on a context of its own; a 32-byte point
// type through the impl header; without a model the input comes back with the identity.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "wave/matching/correspondence_rejection.hpp"
#include "wave/matching/fpfh.hpp"
#include "wave/matching/impl/correspondence_rejection.hpp"
#include "wavematch.h"

struct alignas(16) Point32 {  // x, y, z first, then a payload
    float x, y, z, pad;
    float intensity, ring, a, b;
};
static_assert(sizeof(Point32) == 32, "32-byte point");
template class wave::CorrespondenceRejectorSampleConsensus<Point32>;

static int failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failed;                                                   \
        }                                                               \
    } while (0)

using Cloud = pcl::PointCloud<pcl::PointXYZ>;
using Corrs = std::vector<pcl::Correspondence>;

static bool sameCorrs(const Corrs &a, const Corrs &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].index_query != b[i].index_query || a[i].index_match != b[i].index_match ||
            std::memcmp(&a[i].distance, &b[i].distance, sizeof(float)) != 0)
            return false;
    return true;
}
static bool isIdentity(const Eigen::Matrix4d &m) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            if (m(r, c) != (r == c ? 1.0 : 0.0)) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string scan = argv[1], config = argv[2];
    auto full = boost::make_shared<Cloud>();
    if (pcl::io::loadPCDFile(scan, *full) != 0) return 3;
    // every fourth finite point of the scan; the target is the source moved by 20 degrees of yaw and (0.8, 0.6, 0)
    auto source = boost::make_shared<Cloud>(), target = boost::make_shared<Cloud>();
    const double yaw = 20.0 * 3.14159265358979323846 / 180.0, cs = std::cos(yaw), sn = std::sin(yaw);
    for (size_t i = 0; i < full->size(); i += 4) {
        const auto &q = full->points[i];
        if (!(std::isfinite(q.x) && std::isfinite(q.y) && std::isfinite(q.z))) continue;
        source->push_back(q);
        pcl::PointXYZ t;
        t.x = (float) (cs * q.x - sn * q.y + 0.8);
        t.y = (float) (sn * q.x + cs * q.y + 0.6);
        t.z = q.z;
        target->push_back(t);
    }
    const size_t n = source->size();

    // descriptors of both clouds, matched in descriptor space
    wave::FPFHEstimation<pcl::PointXYZ> fe;
    std::vector<pcl::FPFHSignature33> ds, dt;
    fe.setInputCloud(source);
    fe.compute(ds);
    fe.setInputCloud(target);
    fe.compute(dt);
    Corrs corr;
    CHECK(ds.size() == n && dt.size() == n && wave::matchFeatures(ds, dt, true, corr) && corr.size() > n / 10);

    const wave::CorrespondenceRejectionParams params{config};
    CHECK(params.inlier_threshold == 0.1 && params.max_iterations == 400 && params.probability == 0.99 &&
          params.refine_model == 1 && params.min_sample_distance == -1.0 && params.seed == 0);
    wave::CorrespondenceRejectorSampleConsensus<pcl::PointXYZ> rej{params};
    CHECK(isIdentity(rej.getBestTransformation()) && rej.getRefineModel() && rej.getMaximumIterations() == 400);
    rej.setInputSource(source);
    rej.setInputTarget(target);
    Corrs kept;
    rej.getRemainingCorrespondences(corr, kept);
    const Eigen::Matrix4d T = rej.getBestTransformation();

    // the C ABI on the same correspondences
    wm_ctx *ctx = nullptr;
    if (wm_ctx_create(&ctx, 0) != WM_OK) return 4;
    wm_corr_ransac_params p;
    wm_corr_ransac_default_params(&p);
    CHECK(p.inlier_threshold == 0.05 && p.max_iterations == 1000 && p.probability == 0.99 && p.refine_model == 0 &&
          p.min_sample_distance == -1.0 && p.seed == 0);
    p.inlier_threshold = params.inlier_threshold;
    p.max_iterations = params.max_iterations;
    p.refine_model = params.refine_model;
    std::vector<int32_t> qi(corr.size()), mi(corr.size()), idx(corr.size());
    for (size_t e = 0; e < corr.size(); ++e) qi[e] = corr[e].index_query, mi[e] = corr[e].index_match;
    double Tc[16];
    size_t n_out = 0;
    wm_corr_ransac_stats st;
    CHECK(wm_corr_ransac(ctx, source->points.data(), n, target->points.data(), n, sizeof(pcl::PointXYZ), qi.data(), mi.data(),
                         corr.size(), WM_MEM_HOST, &p, Tc, idx.data(), idx.size(), WM_MEM_HOST, &n_out, nullptr, &st) == WM_OK);
    CHECK(n_out == kept.size() && st.refined == 1 && st.n_valid == corr.size());
    bool same = n_out == kept.size();
    for (size_t k = 0; same && k < n_out; ++k) same = sameCorrs(Corrs(1, kept[k]), Corrs(1, corr[(size_t) idx[k]]));
    CHECK(same);
    CHECK(std::memcmp(T.data(), Tc, sizeof(Tc)) == 0);
    // the pose: 20 degrees of yaw and (0.8, 0.6, 0)
    CHECK(std::fabs(T(0, 0) - cs) < 1e-3 && std::fabs(T(1, 0) - sn) < 1e-3 && std::fabs(T(2, 2) - 1) < 1e-3 &&
          std::fabs(T(0, 3) - 0.8) < 0.02 && std::fabs(T(1, 3) - 0.6) < 0.02 && std::fabs(T(2, 3)) < 0.02 && kept.size() > corr.size() / 2);
    std::printf("%zu points, %zu correspondences, %zu kept; %d iterations, %d skipped; %.3f ms on the device\n", n, corr.size(),
                kept.size(), st.iterations, st.skipped, st.kernel_ms);

    // a copy has its own context; assignment too; setters reach the device
    auto copy = rej;
    Corrs a, b;
    copy.getRemainingCorrespondences(corr, a);
    rej.getRemainingCorrespondences(corr, b);
    CHECK(sameCorrs(a, kept) && sameCorrs(b, kept) && std::memcmp(copy.getBestTransformation().data(), Tc, sizeof(Tc)) == 0);
    wave::CorrespondenceRejectorSampleConsensus<pcl::PointXYZ> assigned;
    assigned = rej;
    assigned.getRemainingCorrespondences(corr, a);
    CHECK(sameCorrs(a, kept));
    assigned.setRefineModel(false);
    assigned.setSeed(5);
    assigned.getRemainingCorrespondences(corr, a);
    CHECK(!a.empty() && std::memcmp(assigned.getBestTransformation().data(), Tc, sizeof(Tc)) != 0);
    a = corr;  // `remaining` may be the input
    rej.getRemainingCorrespondences(a, a);
    CHECK(sameCorrs(a, kept));

    // a 32-byte point type (stride 32): the same bytes
    auto s32 = boost::make_shared<pcl::PointCloud<Point32>>(), t32 = boost::make_shared<pcl::PointCloud<Point32>>();
    for (const auto &q : source->points) s32->push_back(Point32{q.x, q.y, q.z, 1.f, 7.f, 3.f, -1.f, 2.f});
    for (const auto &q : target->points) t32->push_back(Point32{q.x, q.y, q.z, 1.f, 7.f, 3.f, -1.f, 2.f});
    wave::CorrespondenceRejectorSampleConsensus<Point32> r32{params};
    r32.setInputSource(s32);
    r32.setInputTarget(t32);
    r32.getRemainingCorrespondences(corr, a);
    CHECK(sameCorrs(a, kept) && std::memcmp(r32.getBestTransformation().data(), Tc, sizeof(Tc)) == 0);

    // no model: the input comes back with the identity -- every source point of the correspondences the same (every sample
    // is skipped), two correspondences, indices out of range, bad parameters, no clouds
    Corrs flat = corr;
    for (auto &c : flat) c.index_query = 7;
    rej.getRemainingCorrespondences(flat, a);
    CHECK(sameCorrs(a, flat) && isIdentity(rej.getBestTransformation()));
    const Corrs two(corr.begin(), corr.begin() + 2);
    rej.getRemainingCorrespondences(two, a);
    CHECK(sameCorrs(a, two) && isIdentity(rej.getBestTransformation()));
    Corrs wild = corr;
    for (auto &c : wild) c.index_match = (int) n + 5;
    rej.getRemainingCorrespondences(wild, a);
    CHECK(sameCorrs(a, wild) && isIdentity(rej.getBestTransformation()));
    rej.getRemainingCorrespondences(corr, a);  // ... and the object still works
    CHECK(sameCorrs(a, kept));
    rej.setInlierThreshold(0.0);
    rej.getRemainingCorrespondences(corr, a);
    CHECK(sameCorrs(a, corr) && isIdentity(rej.getBestTransformation()));
    wave::CorrespondenceRejectorSampleConsensus<pcl::PointXYZ> none;
    none.getRemainingCorrespondences(corr, a);
    CHECK(sameCorrs(a, corr) && isIdentity(none.getBestTransformation()));

    wm_ctx_destroy(ctx);
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
