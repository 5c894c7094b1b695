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

bool sacSegment(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride, const SACSegmentationParams &params,
                pcl::PointIndices &inliers, pcl::ModelCoefficients &coefficients) {
    inliers.indices.clear();
    coefficients.values.clear();
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

}  // namespace detail

template class SACSegmentation<pcl::PointXYZ>;

}  // namespace wave
