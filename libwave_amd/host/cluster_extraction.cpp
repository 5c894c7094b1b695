// wave::EuclideanClusterExtraction's non-template part and its pcl::PointXYZ instantiation.
#include "wave/matching/cluster_extraction.hpp"

#include <climits>

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

bool clusterExtractBatch(wm_ctx *&ctx, int device, const std::vector<const void *> &pts, const std::vector<size_t> &n,
                         size_t stride, const ClusterExtractionParams &params,
                         std::vector<std::vector<pcl::PointIndices>> &out) {
    out.clear();
    const size_t S = pts.size();
    std::vector<wm_cluster_scan> scans(S);
    size_t total = 0;
    for (size_t k = 0; k < S; ++k) {
        if (n[k] == static_cast<size_t>(-1)) {
            LOG_ERROR("extractBatch: cloud %zu is a null pointer", k);
            return false;
        }
        scans[k].pts = pts[k];
        scans[k].n = n[k];
        total += n[k];
    }
    if (S == 0) return true;
    if (S > (size_t) INT_MAX) {
        LOG_ERROR("extractBatch: too many clouds");
        return false;
    }
    wm_cluster_params p;
    wm_cluster_default_params(&p);
    p.tolerance = params.tolerance;
    p.min_cluster_size = params.min_cluster_size;
    p.max_cluster_size = params.max_cluster_size;
    if (!shim::acquire(ctx, device)) return false;
    std::vector<int32_t> indices(total);
    std::vector<uint32_t> offsets(total + 1);
    std::vector<size_t> first(S + 1);
    size_t n_out = 0;
    const int rc = wm_cluster_extract_batch(ctx, scans.data(), (int) S, stride, WM_MEM_HOST, &p, nullptr,
                                            total ? indices.data() : nullptr, total, nullptr, 0, offsets.data(), total,
                                            WM_MEM_HOST, first.data(), &n_out, nullptr, nullptr);
    if (rc != WM_OK) {
        LOG_ERROR("wm_cluster_extract_batch failed: %s [%s]", wm_strerror(rc), wm_last_error(ctx));
        return false;
    }
    out.resize(S);
    for (size_t k = 0; k < S; ++k) {
        out[k].resize(first[k + 1] - first[k]);
        for (size_t c = first[k]; c < first[k + 1]; ++c)
            out[k][c - first[k]].indices.assign(indices.begin() + offsets[c], indices.begin() + offsets[c + 1]);
    }
    return true;
}

}  // namespace detail

template class EuclideanClusterExtraction<pcl::PointXYZ>;

}  // namespace wave
