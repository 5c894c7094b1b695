// wave::OutlierRemoval's non-template part and its pcl::PointXYZ instantiation.
#include "wave/matching/outlier_removal.hpp"

#include "shim.hpp"
#include "wave/matching/impl/outlier_removal.hpp"

namespace wave {

OutlierRemovalParams::OutlierRemovalParams(const std::string &config_path) {
    try {
        shim::loadYaml(config_path, {{"method", &method},
                                     {"mean_k", &mean_k},
                                     {"stddev_mult", &stddev_mult},
                                     {"radius", &radius},
                                     {"min_neighbors", &min_neighbors},
                                     {"negative", &negative}});
    } catch (const std::runtime_error &) {
        LOG_ERROR("Unable to load config");  // (as GroundSegmentationParams: log and carry on with what is there)
    }
}

namespace detail {

int outlierDefaultDevice() { return shim::defaultDevice(); }

void outlierRelease(wm_ctx *&ctx) { shim::release(ctx); }

bool outlierIndices(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride,
                    const OutlierRemovalParams &params, std::vector<int> &out) {
    out.clear();
    wm_outlier_params p;
    wm_outlier_default_params(&p);
    p.method = params.method;
    p.mean_k = params.mean_k;
    p.stddev_mult = params.stddev_mult;
    p.radius = params.radius;
    p.min_neighbors = params.min_neighbors;
    p.negative = params.negative;
    if (!shim::acquire(ctx, device)) return false;
    out.resize(n);
    size_t m = 0;
    const int rc = wm_outlier_filter(ctx, pts, n, stride, WM_MEM_HOST, &p,
                                     n ? reinterpret_cast<int32_t *>(out.data()) : nullptr, n, WM_MEM_HOST, &m, nullptr,
                                     nullptr, nullptr, nullptr);
    if (rc != WM_OK) {
        LOG_ERROR("wm_outlier_filter failed: %s [%s]", wm_strerror(rc), wm_last_error(ctx));
        out.clear();
        return false;
    }
    out.resize(m);
    return true;
}

}  // namespace detail

template class OutlierRemoval<pcl::PointXYZ>;

}  // namespace wave
