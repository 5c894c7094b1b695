// wave::ConditionalEuclideanClustering<PointT> on the MI355X back end.
//
// pcl::ConditionalEuclideanClustering's surface: setClusterTolerance / setMinClusterSize / setMaxClusterSize,
// setInputCloud, segment(std::vector<pcl::PointIndices> &).  It is EuclideanClusterExtraction with a test on every
// edge: two points closer than the tolerance are joined only if their normals agree (setMaxNormalAngle) and / or
// their scalars -- a curvature, an intensity -- are close (setMaxScalarDifference).  That keeps a parked car apart
// from the wall it stands against.  One segment() is one C-ABI call, wm_cluster_extract_cond (include/wavematch.h,
// which states the rule), preceded by wm_estimate_normals where the class estimates the normals itself.
//
// In place of PCL's setConditionFunction (a caller's function cannot run on the device) there are the two fixed tests,
// both symmetric in their two points; clearConditions() switches both off, and segment() then gives what
// EuclideanClusterExtraction::extract gives.  The attributes (a0, a1, a2, s per point, four floats at the head of a
// record) come from one of two sources:
//   setInputAttributes(attr, n, stride_bytes)  the caller's array, not owned: it must live until segment() returns and
//                                              n must be the input cloud's size;
//   setNormalKSearch(k)                        segment() estimates (nx, ny, nz, curvature) from each point's k nearest
//                                              neighbours, 3 <= k <= 32, on the device: the cloud becomes the source
//                                              and the target of the class's OWN context (nobody else's registration
//                                              state is touched).  Fewer than k finite points is an error.  k > 0
//                                              takes precedence over setInputAttributes; k = 0 switches it off.
// Further differences from PCL's class: the clusters come largest first, equal sizes by their smallest point index,
// not in seed order; a non-finite point is in no cluster; there is no getRemovedClusters, no setSearchMethod and no
// setIndices.  Shaped like wave::EuclideanClusterExtraction<PointT>: the device context is created by the first
// segment(), so construction needs no device; a copy opens a context of its own; bad parameters, missing attributes
// or a device error give a LOG_ERROR and no clusters.  libwave_matching.so holds the pcl::PointXYZ instantiation; any
// other point type whose first three floats are x, y, z works after
// #include <wave/matching/impl/conditional_clustering.hpp>.
#ifndef WAVE_CONDITIONALCLUSTERING_HPP
#define WAVE_CONDITIONALCLUSTERING_HPP

#include <climits>
#include <cstddef>
#include <string>
#include <vector>

#include "wave/compat/pcl_indices_min.hpp"

struct wm_ctx;  // include/wavematch.h

namespace wave {

struct ConditionalClusteringParams {
    ConditionalClusteringParams() {}
    // flat "key: value" YAML file: tolerance, min_cluster_size, max_cluster_size, max_normal_angle, max_scalar_diff,
    // normal_k (libwave_amd/host/conditional_clustering.cpp).  A file that cannot be read logs "Unable to load config"
    // and leaves the defaults, as ClusterExtractionParams does.
    ConditionalClusteringParams(const std::string &config_path);

    double tolerance = 0;            // metres (must be set > 0)
    int min_cluster_size = 1;        // a component with fewer points is dropped (0 acts as 1)
    int max_cluster_size = INT_MAX;  // a component with more points is dropped
    double max_normal_angle = -1;    // radians, 0 ... pi/2; negative: no normal test
    double max_scalar_diff = -1;     // >= 0; negative: no scalar test
    int normal_k = 0;                // > 0: segment() estimates the normals from this many neighbours
};

namespace detail {
// libwave_amd/host/conditional_clustering.cpp: the non-template part of segment
int condClusterDefaultDevice();
void condClusterRelease(wm_ctx *&ctx);
// false (after a LOG_ERROR, `out` empty) on bad parameters, missing attributes or a device error
bool condClusterSegment(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride,
                        const ConditionalClusteringParams &params, bool normal_test, bool scalar_test, const float *attr,
                        size_t attr_n, size_t attr_stride, std::vector<pcl::PointIndices> &out);
}  // namespace detail

template <typename PointT>
class ConditionalEuclideanClustering {
 public:
    using PointCloud = pcl::PointCloud<PointT>;
    using PointCloudConstPtr = typename PointCloud::ConstPtr;

    ConditionalEuclideanClustering();  // PCL's defaults, no test; no device is opened here
    explicit ConditionalEuclideanClustering(const ConditionalClusteringParams &config);
    ConditionalEuclideanClustering(const ConditionalEuclideanClustering &other);  // the copy opens a context of its own
    ConditionalEuclideanClustering &operator=(const ConditionalEuclideanClustering &other);
    ~ConditionalEuclideanClustering();

    void setClusterTolerance(double tolerance) { params.tolerance = tolerance; }
    double getClusterTolerance() const { return params.tolerance; }
    void setMinClusterSize(int min_cluster_size) { params.min_cluster_size = min_cluster_size; }
    int getMinClusterSize() const { return params.min_cluster_size; }
    void setMaxClusterSize(int max_cluster_size) { params.max_cluster_size = max_cluster_size; }
    int getMaxClusterSize() const { return params.max_cluster_size; }

    // each enables its test (a value outside the header's range makes segment() fail, it is not clamped)
    void setMaxNormalAngle(double radians) {
        params.max_normal_angle = radians;
        normal_test = true;
    }
    double getMaxNormalAngle() const { return params.max_normal_angle; }
    void setMaxScalarDifference(double diff) {
        params.max_scalar_diff = diff;
        scalar_test = true;
    }
    double getMaxScalarDifference() const { return params.max_scalar_diff; }
    bool hasNormalTest() const { return normal_test; }
    bool hasScalarTest() const { return scalar_test; }
    void clearConditions() { normal_test = scalar_test = false; }

    void setInputAttributes(const float *attr, size_t n, size_t stride_bytes = 16) {
        attr_ = attr;
        attr_n = n;
        attr_stride = stride_bytes;
    }
    void setNormalKSearch(int k) { params.normal_k = k; }
    int getNormalKSearch() const { return params.normal_k; }

    void setInputCloud(const PointCloudConstPtr &cloud) { input_ = cloud; }
    const PointCloudConstPtr getInputCloud() const { return input_; }

    // the clusters of input_ (wm_cluster_extract_cond), largest first, each one's indices ascending
    void segment(std::vector<pcl::PointIndices> &clusters);

 private:
    PointCloudConstPtr input_;
    ConditionalClusteringParams params;
    bool normal_test = false, scalar_test = false;
    const float *attr_ = nullptr;  // not owned
    size_t attr_n = 0, attr_stride = 16;
    wm_ctx *ctx = nullptr;  // created by the first segment
    int device = 0;
};

}  // namespace wave

#endif  // WAVE_CONDITIONALCLUSTERING_HPP
