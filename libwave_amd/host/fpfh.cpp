// wave::FPFHEstimation's non-template part, its pcl::PointXYZ instantiation, and wave::matchFeatures.
#include "wave/matching/fpfh.hpp"

#include <cstring>

#include "shim.hpp"
#include "wave/matching/impl/fpfh.hpp"

namespace wave {

FPFHParams::FPFHParams(const std::string &config_path) {
    // the k pair, the radius pair or both: a file with neither is no FPFH config
    bool any = false;
    try {
        shim::loadYaml(config_path, {{"feature_k", &feature_k}, {"normal_k", &normal_k}});
        any = true;
    } catch (const std::runtime_error &) {
    }
    try {
        shim::loadYaml(config_path, {{"feature_radius", &feature_radius}, {"normal_radius", &normal_radius}});
        any = true;
    } catch (const std::runtime_error &) {
    }
    if (!any) LOG_ERROR("Unable to load config");  // (as ConditionalClusteringParams: log and carry on with what is there)
}

namespace detail {

int fpfhDefaultDevice() { return shim::defaultDevice(); }

void fpfhRelease(wm_ctx *&ctx) { shim::release(ctx); }

bool fpfhCompute(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride, const FPFHParams &params, bool k_set,
                 bool normal_k_set, const float *normals, size_t normals_n, size_t normals_stride,
                 std::vector<pcl::FPFHSignature33> &out) {
    out.clear();
    const bool radius = params.feature_radius != 0;
    if (radius && k_set) {  // (pcl::Feature::initCompute: "Both radius and K defined!")
        LOG_ERROR("compute: both a radius (%g) and k (%d) are set; set one of them to 0", params.feature_radius, params.feature_k);
        return false;
    }
    if (!radius && params.normal_radius != 0) {
        LOG_ERROR("compute: a normal radius (%g) needs setRadiusSearch; with k the normals come from setNormalKSearch",
                  params.normal_radius);
        return false;
    }
    if (radius && !normals && (normal_k_set || !(params.normal_radius > 0))) {
        LOG_ERROR("compute: with a radius the normals come from setInputNormals or setNormalRadiusSearch (normal_radius = %g%s)",
                  params.normal_radius, normal_k_set ? ", and a normal k is set" : "");
        return false;
    }
    if (!radius && (params.feature_k < 3 || params.feature_k > 32 || params.normal_k < 3 || params.normal_k > 32)) {
        LOG_ERROR("compute: feature_k = %d and normal_k = %d must be 3 ... 32", params.feature_k, params.normal_k);
        return false;
    }
    std::vector<float> packed;  // the caller's normals as the C ABI wants them: float x 4 per point
    if (normals) {
        if (normals_n != n || normals_stride < 3 * sizeof(float) || normals_stride % 4 != 0) {
            LOG_ERROR("compute: %zu normals of stride %zu for a cloud of %zu points", normals_n, normals_stride, n);
            return false;
        }
        packed.assign(4 * n, 0.f);
        for (size_t i = 0; i < n; ++i)
            std::memcpy(&packed[4 * i], reinterpret_cast<const char *>(normals) + i * normals_stride, 3 * sizeof(float));
    }
    if (!shim::acquire(ctx, device)) return false;
    std::vector<float> rows((size_t) WM_FEATURE_DIM * n);
    if (radius) {  // cloud in, rows out: nothing is set on the context
        wm_fpfh_radius_params rp;
        rp.normal_radius = params.normal_radius;
        rp.feature_radius = params.feature_radius;
        wm_fpfh_radius_stats st;
        const int rc = wm_fpfh_radius(ctx, pts, n, stride, WM_MEM_HOST, &rp, normals ? packed.data() : nullptr, rows.data(), nullptr,
                                      nullptr, WM_MEM_HOST, &st);
        if (rc != WM_OK) {  // (WM_ERR_ARG: a bad radius, or a point with more neighbours than the call takes)
            LOG_ERROR("wm_fpfh_radius (feature_radius = %g, normal_radius = %g) failed: %s [%s]; most neighbours of a point: %zu of %d",
                      rp.feature_radius, rp.normal_radius, wm_strerror(rc), wm_last_error(ctx), st.max_neighbors,
                      WM_FPFH_RADIUS_MAX_NEIGHBORS);
            return false;
        }
        out.resize(n);
        for (size_t i = 0; i < n; ++i) std::memcpy(out[i].histogram, &rows[WM_FEATURE_DIM * i], WM_FEATURE_DIM * sizeof(float));
        return true;
    }
    // the cloud as both clouds of this object's own context: the descriptors are the target's
    int rc = wm_set_source(ctx, pts, n, stride, WM_MEM_HOST);
    if (rc == WM_OK) rc = wm_set_target(ctx, pts, n, stride, WM_MEM_HOST);
    if (rc != WM_OK) {
        LOG_ERROR("compute: the cloud could not be set: %s [%s]", wm_strerror(rc), wm_last_error(ctx));
        return false;
    }
    wm_fpfh_params p;
    wm_fpfh_default_params(&p);
    p.feature_k = params.feature_k;
    p.normal_k = params.normal_k;
    rc = wm_fpfh_estimate(ctx, 1, &p, normals ? packed.data() : nullptr, rows.data(), nullptr, WM_MEM_HOST, nullptr);
    if (rc != WM_OK) {  // (WM_NOT_CONVERGED: fewer finite points than neighbours)
        LOG_ERROR("wm_fpfh_estimate (feature_k = %d, normal_k = %d) failed: %s [%s]", p.feature_k, p.normal_k, wm_strerror(rc),
                  wm_last_error(ctx));
        return false;
    }
    out.resize(n);
    for (size_t i = 0; i < n; ++i) std::memcpy(out[i].histogram, &rows[WM_FEATURE_DIM * i], WM_FEATURE_DIM * sizeof(float));
    return true;
}

}  // namespace detail

bool matchFeatures(const std::vector<pcl::FPFHSignature33> &a, const std::vector<pcl::FPFHSignature33> &b, bool reciprocal,
                   std::vector<pcl::Correspondence> &out) {
    static_assert(sizeof(pcl::FPFHSignature33) >= WM_FEATURE_DIM * sizeof(float) && sizeof(pcl::FPFHSignature33) % 4 == 0,
                  "a descriptor record begins with its 33 floats");
    out.clear();
    if (a.empty()) return true;
    if (a.size() > WM_FEATURE_MAX_ROWS || b.size() > WM_FEATURE_MAX_ROWS) {
        LOG_ERROR("matchFeatures: %zu and %zu descriptors, at most %u per side", a.size(), b.size(), WM_FEATURE_MAX_ROWS);
        return false;
    }
    wm_ctx *ctx = nullptr;
    if (!shim::acquire(ctx, shim::defaultDevice())) return false;
    std::vector<int32_t> idx(a.size());
    std::vector<float> d2(a.size());
    const int rc = wm_feature_match(ctx, a.data(), a.size(), sizeof(pcl::FPFHSignature33), b.empty() ? nullptr : b.data(), b.size(),
                                    sizeof(pcl::FPFHSignature33), WM_MEM_HOST, reciprocal ? 1 : 0, idx.data(), d2.data(),
                                    WM_MEM_HOST, nullptr);
    if (rc != WM_OK) LOG_ERROR("wm_feature_match failed: %s [%s]", wm_strerror(rc), wm_last_error(ctx));
    shim::release(ctx);
    if (rc != WM_OK) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (idx[i] >= 0) {
            pcl::Correspondence c;
            c.index_query = (int) i;
            c.index_match = idx[i];
            c.distance = d2[i];
            out.push_back(c);
        }
    return true;
}

template class FPFHEstimation<pcl::PointXYZ>;

}  // namespace wave
