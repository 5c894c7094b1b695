// wave::FPFHEstimation<pcl::PointXYZ> and wave::matchFeatures on the scan fixture with the YAML fixture's parameters:
// compute() against the bytes the C ABI (wm_fpfh_estimate, called here on a context of its own) gives for the same
// cloud; the caller's normals (setInputNormals, a stride of 32) against estimated ones; a copy works on a context of its
// own; a 32-byte point type through the impl header; matchFeatures against wm_feature_match minus the unmatched rows,
// plain and reciprocal; bad parameters and missing normals give an empty result.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "wave/matching/fpfh.hpp"
#include "wave/matching/impl/fpfh.hpp"
#include "wavematch.h"

struct alignas(16) Point32 {  // x, y, z first, then a payload
    float x, y, z, pad;
    float intensity, ring, a, b;
};
static_assert(sizeof(Point32) == 32, "32-byte point");
template class wave::FPFHEstimation<Point32>;

static int failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failed;                                                   \
        }                                                               \
    } while (0)

using Cloud = pcl::PointCloud<pcl::PointXYZ>;
using Descriptors = std::vector<pcl::FPFHSignature33>;

static bool sameRows(const Descriptors &a, const std::vector<float> &rows) {
    if (a.size() * 33 != rows.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (std::memcmp(a[i].histogram, &rows[33 * i], 33 * sizeof(float)) != 0) return false;
    return true;
}
static bool sameRows(const Descriptors &a, const Descriptors &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (std::memcmp(a[i].histogram, b[i].histogram, 33 * sizeof(float)) != 0) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string scan = argv[1], config = argv[2];
    auto input = boost::make_shared<Cloud>();
    if (pcl::io::loadPCDFile(scan, *input) != 0) return 3;
    const size_t n = input->size();
    wm_ctx *ctx = nullptr;
    if (wm_ctx_create(&ctx, 0) != WM_OK) return 4;

    const wave::FPFHParams params{config};
    CHECK(params.feature_k == 12 && params.normal_k == 16);
    wave::FPFHEstimation<pcl::PointXYZ> fe{params};
    fe.setInputCloud(input);
    CHECK(fe.getInputCloud() == input && fe.getKSearch() == 12 && fe.getNormalKSearch() == 16);
    Descriptors got;
    fe.compute(got);

    // the C ABI on the same cloud
    wm_fpfh_params p;
    wm_fpfh_default_params(&p);
    CHECK(p.feature_k == 10 && p.normal_k == 10);
    p.feature_k = params.feature_k;
    p.normal_k = params.normal_k;
    std::vector<float> want(33 * n), normals(4 * n);
    wm_fpfh_stats st;
    CHECK(wm_set_source(ctx, input->points.data(), n, sizeof(pcl::PointXYZ), WM_MEM_HOST) == WM_OK);
    CHECK(wm_set_target(ctx, input->points.data(), n, sizeof(pcl::PointXYZ), WM_MEM_HOST) == WM_OK);
    CHECK(wm_fpfh_estimate(ctx, 1, &p, nullptr, want.data(), nullptr, WM_MEM_HOST, &st) == WM_OK);
    CHECK(wm_estimate_normals(ctx, 1, params.normal_k, normals.data(), WM_MEM_HOST) == WM_OK);
    CHECK(got.size() == n && sameRows(got, want) && st.n_valid > n / 2 && st.n_valid <= n);
    std::printf("%zu points, %zu valid descriptors; device ms: normals %.3f, first pass %.3f, second pass %.3f\n", n, st.n_valid,
                st.normals_ms, st.spfh_ms, st.weight_ms);

    // the caller's normals in records of 32 bytes: the same descriptors
    std::vector<float> wide(8 * n, 7.f);
    for (size_t i = 0; i < n; ++i) std::memcpy(&wide[8 * i], &normals[4 * i], 3 * sizeof(float));
    fe.setInputNormals(wide.data(), n, 32);
    Descriptors given;
    fe.compute(given);
    CHECK(sameRows(given, got));
    fe.setInputNormals(wide.data(), n - 1, 32);  // not the cloud's size
    fe.compute(given);
    CHECK(given.empty());
    fe.setInputNormals(nullptr, 0);

    // a copy has its own context; assignment too; setters reach the device
    auto copy = fe;
    Descriptors a, b;
    copy.compute(a);
    fe.compute(b);
    CHECK(sameRows(a, got) && sameRows(b, got));
    wave::FPFHEstimation<pcl::PointXYZ> assigned;
    assigned = fe;
    assigned.compute(a);
    CHECK(sameRows(a, got));
    assigned.setKSearch(10);
    assigned.compute(a);
    CHECK(a.size() == n && !sameRows(a, got));
    assigned.setKSearch(33);
    assigned.compute(a);
    CHECK(a.empty());
    assigned.setKSearch(12);
    assigned.setNormalKSearch(2);
    assigned.compute(a);
    CHECK(a.empty());

    // a 32-byte point type (stride 32): the same bytes
    auto in32 = boost::make_shared<pcl::PointCloud<Point32>>();
    for (const auto &q : input->points) in32->push_back(Point32{q.x, q.y, q.z, 1.f, 7.f, 3.f, -1.f, 2.f});
    wave::FPFHEstimation<Point32> f32{params};
    f32.setInputCloud(in32);
    f32.compute(a);
    CHECK(sameRows(a, got));

    // no cloud, an empty cloud: nothing
    wave::FPFHEstimation<pcl::PointXYZ> none;
    none.compute(a);
    CHECK(a.empty());
    none.setInputCloud(boost::make_shared<Cloud>());
    none.compute(a);
    CHECK(a.empty());

    // matchFeatures: the first half's descriptors against the second half's
    const Descriptors da(got.begin(), got.begin() + n / 2), db(got.begin() + n / 2, got.end());
    for (int reciprocal = 0; reciprocal < 2; ++reciprocal) {
        std::vector<pcl::Correspondence> corr;
        CHECK(wave::matchFeatures(da, db, reciprocal != 0, corr));
        std::vector<int32_t> idx(da.size());
        std::vector<float> d2(da.size());
        wm_feature_match_stats ms;
        CHECK(wm_feature_match(ctx, da.data(), da.size(), sizeof(pcl::FPFHSignature33), db.data(), db.size(),
                               sizeof(pcl::FPFHSignature33), WM_MEM_HOST, reciprocal, idx.data(), d2.data(), WM_MEM_HOST,
                               &ms) == WM_OK);
        size_t k = 0;
        bool same = true;
        for (size_t i = 0; i < idx.size(); ++i)
            if (idx[i] >= 0) {
                same = same && k < corr.size() && corr[k].index_query == (int) i && corr[k].index_match == idx[i] &&
                       std::memcmp(&corr[k].distance, &d2[i], sizeof(float)) == 0;
                ++k;
            }
        CHECK(same && k == corr.size() && ms.n_matched == corr.size() && !corr.empty());
        std::printf("%zu x %zu descriptors, reciprocal %d: %zu correspondences, %.3f ms on the device\n", da.size(), db.size(),
                    reciprocal, corr.size(), ms.kernel_ms);
    }
    std::vector<pcl::Correspondence> corr(3);
    CHECK(wave::matchFeatures(Descriptors(), db, false, corr) && corr.empty());
    CHECK(wave::matchFeatures(da, Descriptors(), true, corr) && corr.empty());

    wm_ctx_destroy(ctx);
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
