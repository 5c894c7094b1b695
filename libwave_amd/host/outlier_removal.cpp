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

namespace {

wm_outlier_params outlierParams(const OutlierRemovalParams &params) {
    wm_outlier_params p;
    wm_outlier_default_params(&p);
    p.method = params.method;
    p.mean_k = params.mean_k;
    p.stddev_mult = params.stddev_mult;
    p.radius = params.radius;
    p.min_neighbors = params.min_neighbors;
    p.negative = params.negative;
    return p;
}

}  // namespace

bool outlierIndices(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride,
                    const OutlierRemovalParams &params, std::vector<int> &out) {
    out.clear();
    const wm_outlier_params p = outlierParams(params);
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

bool outlierIndicesBatch(wm_ctx *&ctx, int device, const void *const *pts, const size_t *n, const unsigned char *null_cloud,
                         size_t count, size_t stride, const OutlierRemovalParams &params,
                         std::vector<std::vector<int>> &out) {
    out.assign(count, std::vector<int>());
    const wm_outlier_params p = outlierParams(params);
    std::vector<wm_outlier_scan> scans(count);
    size_t total = 0;
    for (size_t k = 0; k < count; ++k) {
        if (null_cloud[k]) LOG_ERROR("filterBatch: cloud %zu is a null pointer", k);
        scans[k].pts = pts[k];
        scans[k].n = n[k];
        total += n[k];
    }
    if (count > WM_OUTLIER_BATCH_MAX_SCANS) {
        LOG_ERROR("filterBatch: too many clouds");
        return false;
    }
    if (total == 0) return true;  // (nothing to filter: no device is opened)
    if (!shim::acquire(ctx, device)) return false;
    std::vector<int32_t> idx(total);
    std::vector<size_t> offsets(count + 1, 0);
    std::vector<int> status(count, WM_OK);
    const int rc = wm_outlier_filter_batch(ctx, scans.data(), static_cast<int>(count), stride, WM_MEM_HOST, &p, idx.data(),
                                           total, nullptr, 0, WM_MEM_HOST, offsets.data(), nullptr, nullptr, nullptr,
                                           status.data(), nullptr, nullptr);
    if (rc != WM_OK) {
        LOG_ERROR("wm_outlier_filter_batch failed: %s [%s]", wm_strerror(rc), wm_last_error(ctx));
        return false;
    }
    for (size_t k = 0; k < count; ++k) {
        if (status[k] != WM_OK) {  // (as filter() for that cloud alone: logged, an empty output)
            LOG_ERROR("wm_outlier_filter_batch: cloud %zu failed: %s", k, wm_strerror(status[k]));
            continue;
        }
        out[k].assign(idx.begin() + offsets[k], idx.begin() + offsets[k + 1]);
    }
    return true;
}

}  // namespace detail

template class OutlierRemoval<pcl::PointXYZ>;

}  // namespace wave
