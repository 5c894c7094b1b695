// wave::ConditionalEuclideanClustering's non-template part and its pcl::PointXYZ instantiation.
#include "wave/matching/conditional_clustering.hpp"

#include <climits>

#include "shim.hpp"
#include "wave/matching/impl/conditional_clustering.hpp"

namespace wave {

ConditionalClusteringParams::ConditionalClusteringParams(const std::string &config_path) {
    try {
        shim::loadYaml(config_path, {{"tolerance", &tolerance},
                                     {"min_cluster_size", &min_cluster_size},
                                     {"max_cluster_size", &max_cluster_size},
                                     {"max_normal_angle", &max_normal_angle},
                                     {"max_scalar_diff", &max_scalar_diff},
                                     {"normal_k", &normal_k}});
    } catch (const std::runtime_error &) {
        LOG_ERROR("Unable to load config");  // (as ClusterExtractionParams: log and carry on with what is there)
    }
}

namespace detail {

int condClusterDefaultDevice() { return shim::defaultDevice(); }

void condClusterRelease(wm_ctx *&ctx) { shim::release(ctx); }

bool condClusterSegment(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride,
                        const ConditionalClusteringParams &params, bool normal_test, bool scalar_test, const float *attr,
                        size_t attr_n, size_t attr_stride, std::vector<pcl::PointIndices> &out) {
    out.clear();
    wm_cluster_params p;
    wm_cluster_default_params(&p);
    p.tolerance = params.tolerance;
    p.min_cluster_size = params.min_cluster_size;
    p.max_cluster_size = params.max_cluster_size;
    wm_cluster_cond c;
    wm_cluster_cond_default(&c);
    if (normal_test) {
        c.flags |= WM_CLUSTER_COND_NORMAL;
        c.max_normal_angle = params.max_normal_angle;
    }
    if (scalar_test) {
        c.flags |= WM_CLUSTER_COND_SCALAR;
        c.max_scalar_diff = params.max_scalar_diff;
    }
    if (!shim::acquire(ctx, device)) return false;
    std::vector<float> normals;  // setNormalKSearch: (nx, ny, nz, curvature) per point, estimated here
    if (c.flags == 0 || n == 0) {
        attr = nullptr;  // (no test reads them)
        attr_stride = 16;
    } else if (params.normal_k > 0) {
        // the cloud as both clouds of this object's own context: wm_estimate_normals wants a registration's pair
        int rc = wm_set_source(ctx, pts, n, stride, WM_MEM_HOST);
        if (rc == WM_OK) rc = wm_set_target(ctx, pts, n, stride, WM_MEM_HOST);
        if (rc != WM_OK) {
            LOG_ERROR("segment: the cloud could not be set: %s [%s]", wm_strerror(rc), wm_last_error(ctx));
            return false;
        }
        normals.resize(4 * n);
        rc = wm_estimate_normals(ctx, 1, params.normal_k, normals.data(), WM_MEM_HOST);
        if (rc != WM_OK) {  // (WM_NOT_CONVERGED: fewer than normal_k finite points)
            LOG_ERROR("wm_estimate_normals (k = %d) failed: %s [%s]", params.normal_k, wm_strerror(rc), wm_last_error(ctx));
            return false;
        }
        attr = normals.data();
        attr_stride = 16;
    } else if (!attr || attr_n != n) {
        LOG_ERROR("segment: a test is enabled, but there are no attributes for the cloud's %zu points "
                  "(setInputAttributes: %zu records; setNormalKSearch: off)", n, attr ? attr_n : (size_t) 0);
        return false;
    }
    std::vector<int32_t> indices(n);
    std::vector<uint32_t> offsets(n + 1);
    size_t n_clusters = 0, n_out = 0;
    const int rc = wm_cluster_extract_cond(ctx, pts, n, stride, WM_MEM_HOST, attr, attr_stride, WM_MEM_HOST, &p, &c, nullptr,
                                           n ? indices.data() : nullptr, n, offsets.data(), n, WM_MEM_HOST, &n_clusters,
                                           &n_out, nullptr);
    if (rc != WM_OK) {
        LOG_ERROR("wm_cluster_extract_cond failed: %s [%s]", wm_strerror(rc), wm_last_error(ctx));
        return false;
    }
    out.resize(n_clusters);
    for (size_t k = 0; k < n_clusters; ++k)
        out[k].indices.assign(indices.begin() + offsets[k], indices.begin() + offsets[k + 1]);
    return true;
}

}  // namespace detail

template class ConditionalEuclideanClustering<pcl::PointXYZ>;

}  // namespace wave
