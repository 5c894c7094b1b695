// wave::EuclideanClusterExtraction's non-template part and its pcl::PointXYZ instantiation.
#include "wave/matching/cluster_extraction.hpp"

#include "shim.hpp"
#include "wave/matching/impl/cluster_extraction.hpp"

namespace wave {

ClusterExtractionParams::ClusterExtractionParams(const std::string &config_path) {
    try {
        shim::loadYaml(config_path, {{"tolerance", &tolerance},
                                     {"min_cluster_size", &min_cluster_size},
                                     {"max_cluster_size", &max_cluster_size}});
    } catch (const std::runtime_error &) {
        LOG_ERROR("Unable to load config");  // (as OutlierRemovalParams: log and carry on with what is there)
    }
}

namespace detail {

int clusterDefaultDevice() { return shim::defaultDevice(); }

void clusterRelease(wm_ctx *&ctx) { shim::release(ctx); }

bool clusterExtract(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride,
                    const ClusterExtractionParams &params, std::vector<pcl::PointIndices> &out) {
    out.clear();
    wm_cluster_params p;
    wm_cluster_default_params(&p);
    p.tolerance = params.tolerance;
    p.min_cluster_size = params.min_cluster_size;
    p.max_cluster_size = params.max_cluster_size;
    if (!shim::acquire(ctx, device)) return false;
    std::vector<int32_t> indices(n);
    std::vector<uint32_t> offsets(n + 1);
    size_t n_clusters = 0, n_out = 0;
    const int rc = wm_cluster_extract(ctx, pts, n, stride, WM_MEM_HOST, &p, nullptr, n ? indices.data() : nullptr, n,
                                      offsets.data(), n, WM_MEM_HOST, &n_clusters, &n_out, nullptr);
    if (rc != WM_OK) {
        LOG_ERROR("wm_cluster_extract failed: %s [%s]", wm_strerror(rc), wm_last_error(ctx));
        return false;
    }
    out.resize(n_clusters);
    for (size_t c = 0; c < n_clusters; ++c)
        out[c].indices.assign(indices.begin() + offsets[c], indices.begin() + offsets[c + 1]);
    return true;
}

}  // namespace detail

template class EuclideanClusterExtraction<pcl::PointXYZ>;

}  // namespace wave
