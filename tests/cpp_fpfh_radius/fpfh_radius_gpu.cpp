// wave::FPFHEstimation<pcl::PointXYZ> with setRadiusSearch on the scan fixture with the radius YAML fixture's parameters:
// compute() against the bytes the C ABI (wm_fpfh_radius, called here on a context of its own) gives for the same cloud;
// the caller's normals (setInputNormals, a stride of 32) against estimated ones; a copy works on a context of its own;
// a 32-byte point type through the impl header; a radius beside a k set by the caller, a normal radius beside a normal
// k, and a radius without any normals give an empty result; setRadiusSearch(0) is back to k.
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
    CHECK(params.feature_radius == 1.0 && params.normal_radius == 0.5 && params.feature_k == 10 && params.normal_k == 10);
    wave::FPFHEstimation<pcl::PointXYZ> fe{params};
    fe.setInputCloud(input);
    CHECK(fe.getRadiusSearch() == 1.0 && fe.getNormalRadiusSearch() == 0.5);
    Descriptors got;
    fe.compute(got);

    // the C ABI on the same cloud: no cloud is set on the context
    wm_fpfh_radius_params p;
    p.feature_radius = params.feature_radius;
    p.normal_radius = params.normal_radius;
    std::vector<float> want(33 * n), normals(4 * n);
    wm_fpfh_radius_stats st;
    CHECK(wm_fpfh_radius(ctx, input->points.data(), n, sizeof(pcl::PointXYZ), WM_MEM_HOST, &p, nullptr, want.data(), nullptr, nullptr,
                         WM_MEM_HOST, &st) == WM_OK);
    CHECK(wm_normals_radius(ctx, input->points.data(), n, sizeof(pcl::PointXYZ), WM_MEM_HOST, p.normal_radius, normals.data(), nullptr,
                            nullptr, WM_MEM_HOST, nullptr) == WM_OK);
    CHECK(got.size() == n && sameRows(got, want) && st.n_valid > n / 2 && st.n_valid <= n && st.max_neighbors > 10);
    std::printf("%zu points, %zu valid descriptors, at most %zu neighbours; device ms: normals %.3f, first walk %.3f, second walk %.3f\n",
                n, st.n_valid, st.max_neighbors, st.normals_ms, st.spfh_ms, st.weight_ms);

    // the caller's normals in records of 32 bytes: the same descriptors, and no normal radius is needed
    std::vector<float> wide(8 * n, 7.f);
    for (size_t i = 0; i < n; ++i) std::memcpy(&wide[8 * i], &normals[4 * i], 3 * sizeof(float));
    fe.setInputNormals(wide.data(), n, 32);
    fe.setNormalRadiusSearch(0.0);
    Descriptors given;
    fe.compute(given);
    CHECK(sameRows(given, got));
    fe.setInputNormals(nullptr, 0);
    fe.compute(given);  // a radius, no normals and no normal radius
    CHECK(given.empty());
    fe.setNormalRadiusSearch(0.5);

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
    assigned.setRadiusSearch(0.7);
    assigned.compute(a);
    CHECK(a.size() == n && !sameRows(a, got));
    assigned.setRadiusSearch(-1.0);
    assigned.compute(a);
    CHECK(a.empty());

    // a radius and a k both set by the caller: PCL's error
    auto both = fe;
    both.setKSearch(12);
    both.compute(a);
    CHECK(a.empty());
    auto both_normals = fe;
    both_normals.setNormalKSearch(12);
    both_normals.compute(a);
    CHECK(a.empty());
    // ... and back to k with the radius at 0: the k form, which knows no normal radius
    both.setRadiusSearch(0.0);
    both.compute(a);
    CHECK(a.empty());
    both.setNormalRadiusSearch(0.0);
    both.compute(a);
    wave::FPFHEstimation<pcl::PointXYZ> kform;
    kform.setInputCloud(input);
    kform.setKSearch(12);
    kform.compute(b);
    CHECK(a.size() == n && sameRows(a, b) && !sameRows(a, got));

    // a 32-byte point type (stride 32): the same bytes
    auto in32 = boost::make_shared<pcl::PointCloud<Point32>>();
    for (const auto &q : input->points) in32->push_back(Point32{q.x, q.y, q.z, 1.f, 7.f, 3.f, -1.f, 2.f});
    wave::FPFHEstimation<Point32> f32{params};
    f32.setInputCloud(in32);
    f32.compute(a);
    CHECK(sameRows(a, got));

    wm_ctx_destroy(ctx);
    std::printf("failed checks: %d\n", failed);
    return failed ? 1 : 0;
}
