// wave::SACSegmentation's non-template part and its pcl::PointXYZ instantiation.
#include "wave/matching/sac_segmentation.hpp"

#include "shim.hpp"
#include "wave/matching/impl/sac_segmentation.hpp"

namespace wave {

SACSegmentationParams::SACSegmentationParams(const std::string &config_path) {
    int optimize = optimize_coefficients ? 1 : 0, seed_value = 0;
    try {
        shim::loadYaml(config_path, {{"model_type", &model_type},
                                     {"distance_threshold", &distance_threshold},
                                     {"max_iterations", &max_iterations},
                                     {"probability", &probability},
                                     {"optimize_coefficients", &optimize},
                                     {"axis_x", &axis[0]},
                                     {"axis_y", &axis[1]},
                                     {"axis_z", &axis[2]},
                                     {"eps_angle", &eps_angle},
                                     {"seed", &seed_value}});
        optimize_coefficients = optimize != 0;
        seed = seed_value < 0 ? 0 : static_cast<uint64_t>(seed_value);
    } catch (const std::runtime_error &) {
        LOG_ERROR("Unable to load config");  // (as ClusterExtractionParams: log and carry on with what is there)
        *this = SACSegmentationParams{};
    }
}

namespace detail {

int sacDefaultDevice() { return shim::defaultDevice(); }

void sacRelease(wm_ctx *&ctx) { shim::release(ctx); }

namespace {

// the C ABI's parameters of `params`; false (after a LOG_ERROR): a method or model that is not built
bool sacParams(const SACSegmentationParams &params, wm_sac_params *out) {
    if (params.method_type != pcl::SAC_RANSAC) {
        LOG_ERROR("SACSegmentation: only SAC_RANSAC is built (method type %d)", params.method_type);
        return false;
    }
    wm_sac_params p;
    wm_sac_default_params(&p);
    switch (params.model_type) {
        case pcl::SACMODEL_PLANE: p.model = WM_SAC_PLANE; break;
        case pcl::SACMODEL_PERPENDICULAR_PLANE: p.model = WM_SAC_PERPENDICULAR_PLANE; break;
        case pcl::SACMODEL_PARALLEL_PLANE: p.model = WM_SAC_PARALLEL_PLANE; break;
        default: LOG_ERROR("SACSegmentation: only the plane models are built (model type %d)", params.model_type); return false;
    }
    p.distance_threshold = params.distance_threshold;
    p.max_iterations = params.max_iterations;
    p.probability = params.probability;
    p.optimize_coefficients = params.optimize_coefficients ? 1 : 0;
    for (int k = 0; k < 3; ++k) p.axis[k] = params.axis[k];
    p.eps_angle = params.eps_angle;
    p.seed = params.seed;
    *out = p;
    return true;
}

}  // namespace

bool sacSegment(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride, const SACSegmentationParams &params,
                pcl::PointIndices &inliers, pcl::ModelCoefficients &coefficients) {
    inliers.indices.clear();
    coefficients.values.clear();
    wm_sac_params p;
    if (!sacParams(params, &p)) return false;
    if (!shim::acquire(ctx, device)) return false;
    std::vector<int32_t> indices(n);
    float coef[4] = {0, 0, 0, 0};
    size_t n_out = 0;
    const int rc = wm_sac_segment(ctx, pts, n, stride, WM_MEM_HOST, &p, coef, n ? indices.data() : nullptr, n, WM_MEM_HOST,
                                  &n_out, nullptr, nullptr);
    if (rc != WM_OK) {
        if (rc == WM_NOT_CONVERGED) LOG_ERROR("wm_sac_segment: no model found");
        else LOG_ERROR("wm_sac_segment failed: %s [%s]", wm_strerror(rc), wm_last_error(ctx));
        return false;
    }
    inliers.indices.assign(indices.begin(), indices.begin() + n_out);
    coefficients.values.assign(coef, coef + 4);
    return true;
}

bool sacSegmentBatch(wm_ctx *&ctx, int device, const void *const *pts, const size_t *n, const unsigned char *null_cloud,
                     size_t count, size_t stride, const SACSegmentationParams &params, std::vector<pcl::PointIndices> &inliers,
                     std::vector<pcl::ModelCoefficients> &coefficients) {
    inliers.assign(count, pcl::PointIndices());
    coefficients.assign(count, pcl::ModelCoefficients());
    wm_sac_params p;
    if (!sacParams(params, &p)) return false;
    std::vector<wm_sac_scan> scans(count);
    size_t total = 0;
    bool any = false;
    for (size_t k = 0; k < count; ++k) {
        if (null_cloud[k]) LOG_ERROR("segmentBatch: cloud %zu is a null pointer", k);
        scans[k].pts = pts[k];
        scans[k].n = n[k];
        total += n[k];
        any = any || n[k] >= 3;
    }
    if (count > WM_SAC_BATCH_MAX_SCANS) {
        LOG_ERROR("segmentBatch: too many clouds");
        return false;
    }
    if (!any) {  // (no cloud has a sample: no device is opened; as segment() for each alone)
        for (size_t k = 0; k < count; ++k)
            if (!null_cloud[k]) LOG_ERROR("wm_sac_segment_batch: cloud %zu: no model found", k);
        return true;
    }
    if (!shim::acquire(ctx, device)) return false;
    std::vector<int32_t> idx(total);
    std::vector<float> coef(4 * count, 0.f);
    std::vector<size_t> offsets(count + 1, 0);
    std::vector<int> status(count, WM_NOT_CONVERGED);
    const int rc = wm_sac_segment_batch(ctx, scans.data(), static_cast<int>(count), stride, WM_MEM_HOST, &p, 0, coef.data(),
                                        idx.data(), total, nullptr, 0, WM_MEM_HOST, offsets.data(), nullptr, status.data(),
                                        nullptr, nullptr);
    if (rc != WM_OK) {
        LOG_ERROR("wm_sac_segment_batch failed: %s [%s]", wm_strerror(rc), wm_last_error(ctx));
        return false;
    }
    for (size_t k = 0; k < count; ++k) {
        if (status[k] != WM_OK) {  // (as segment() for that cloud alone: logged, both outputs empty)
            if (!null_cloud[k]) LOG_ERROR("wm_sac_segment_batch: cloud %zu: no model found", k);
            continue;
        }
        inliers[k].indices.assign(idx.begin() + offsets[k], idx.begin() + offsets[k + 1]);
        coefficients[k].values.assign(coef.begin() + 4 * k, coef.begin() + 4 * k + 4);
    }
    return true;
}

}  // namespace detail

template class SACSegmentation<pcl::PointXYZ>;

}  // namespace wave
