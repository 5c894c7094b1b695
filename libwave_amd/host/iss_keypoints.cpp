// wave::ISSKeypoint3D's non-template part and its pcl::PointXYZ instantiation.
#include "wave/matching/iss_keypoints.hpp"

#include "shim.hpp"
#include "wave/matching/impl/iss_keypoints.hpp"

namespace wave {

ISSKeypointParams::ISSKeypointParams(const std::string &config_path) {
    try {
        shim::loadYaml(config_path, {{"salient_radius", &salient_radius},
                                     {"non_max_radius", &non_max_radius},
                                     {"gamma_21", &gamma_21},
                                     {"gamma_32", &gamma_32},
                                     {"min_neighbors", &min_neighbors}});
    } catch (const std::runtime_error &) {
        LOG_ERROR("Unable to load config");  // (as OutlierRemovalParams: log and carry on with what is there)
    }
}

namespace detail {

int issDefaultDevice() { return shim::defaultDevice(); }

void issRelease(wm_ctx *&ctx) { shim::release(ctx); }

bool issIndices(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride, const ISSKeypointParams &params,
                double border_radius, double normal_radius, std::vector<int> &out) {
    out.clear();
    if (border_radius > 0 || normal_radius > 0) {
        LOG_ERROR("ISSKeypoint3D: the border estimation (setBorderRadius / setNormalRadius > 0) is not built");
        return false;
    }
    wm_iss_params p;
    wm_iss_default_params(&p);
    p.salient_radius = params.salient_radius;
    p.non_max_radius = params.non_max_radius;
    p.gamma_21 = params.gamma_21;
    p.gamma_32 = params.gamma_32;
    p.min_neighbors = params.min_neighbors;
    if (n == 0) return true;  // (nothing to detect: no device is opened)
    if (!shim::acquire(ctx, device)) return false;
    out.resize(n);
    size_t m = 0;
    const int rc = wm_iss_keypoints(ctx, pts, n, stride, WM_MEM_HOST, &p, reinterpret_cast<int32_t *>(out.data()), n, WM_MEM_HOST,
                                    &m, nullptr, nullptr, nullptr, nullptr);
    if (rc != WM_OK) {
        LOG_ERROR("wm_iss_keypoints failed: %s [%s]", wm_strerror(rc), wm_last_error(ctx));
        out.clear();
        return false;
    }
    out.resize(m);
    return true;
}

}  // namespace detail

template class ISSKeypoint3D<pcl::PointXYZ>;

}  // namespace wave
