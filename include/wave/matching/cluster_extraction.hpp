// wave::EuclideanClusterExtraction<PointT> on the MI355X back end.
//
// pcl::EuclideanClusterExtraction's surface: setClusterTolerance / setMinClusterSize / setMaxClusterSize,
// setInputCloud, extract(std::vector<pcl::PointIndices> &).  It splits a cloud -- the obstacle points that
// GroundSegmentation keeps, say -- into objects: the connected components of "closer than the tolerance".  One
// extract() is one C-ABI call, wm_cluster_extract (include/wavematch.h, which states the rule): the neighbour search,
// the components and their order are formed on the device; the host only cuts the index list into clusters.
//
// The reference has no such class (its pipelines call PCL's); this one is shaped like wave::OutlierRemoval<PointT>:
// the device context is created by the first extract(), so construction needs no device; a copy opens a context of
// its own; bad parameters or a device error give a LOG_ERROR and no clusters.  Differences from PCL's class: clusters
// of equal size come in the order of their smallest point index (PCL leaves that to std::sort); a non-finite point is
// nobody's neighbour and is in no cluster; there is no setSearchMethod (the search is the device's grid) and no
// setIndices.  libwave_matching.so holds the pcl::PointXYZ instantiation; any other point type whose first three
// floats are x, y, z works after #include <wave/matching/impl/cluster_extraction.hpp>.
#ifndef WAVE_CLUSTEREXTRACTION_HPP
#define WAVE_CLUSTEREXTRACTION_HPP

#include <climits>
#include <cstddef>
#include <string>
#include <vector>

#include "wave/compat/pcl_indices_min.hpp"

struct wm_ctx;  // include/wavematch.h

namespace wave {

struct ClusterExtractionParams {
    ClusterExtractionParams() {}
    // flat "key: value" YAML file: tolerance, min_cluster_size, max_cluster_size
    // (libwave_amd/host/cluster_extraction.cpp).  A file that cannot be read logs "Unable to load config" and leaves
    // the defaults, as OutlierRemovalParams does.
    ClusterExtractionParams(const std::string &config_path);

    // the defaults are PCL's (wm_cluster_default_params)
    double tolerance = 0;            // metres (must be set > 0)
    int min_cluster_size = 1;        // a component with fewer points is dropped (0 acts as 1)
    int max_cluster_size = INT_MAX;  // a component with more points is dropped
};

namespace detail {
// libwave_amd/host/cluster_extraction.cpp: the non-template part of extract
int clusterDefaultDevice();
void clusterRelease(wm_ctx *&ctx);
// false (after a LOG_ERROR, `out` empty) on bad parameters or a device error
bool clusterExtract(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride,
                    const ClusterExtractionParams &params, std::vector<pcl::PointIndices> &out);
// a queue of clouds in ONE call (wm_cluster_extract_batch): pts[k] / n[k] are cloud k's records; out[k] its clusters
bool clusterExtractBatch(wm_ctx *&ctx, int device, const std::vector<const void *> &pts, const std::vector<size_t> &n,
                         size_t stride, const ClusterExtractionParams &params,
                         std::vector<std::vector<pcl::PointIndices>> &out);
}  // namespace detail

template <typename PointT>
class EuclideanClusterExtraction {
 public:
    using PointCloud = pcl::PointCloud<PointT>;
    using PointCloudConstPtr = typename PointCloud::ConstPtr;

    EuclideanClusterExtraction();                                               // PCL's defaults; no device is opened here
    explicit EuclideanClusterExtraction(const ClusterExtractionParams &config);
    EuclideanClusterExtraction(const EuclideanClusterExtraction &other);        // the copy opens a context of its own
    EuclideanClusterExtraction &operator=(const EuclideanClusterExtraction &other);
    ~EuclideanClusterExtraction();

    void setClusterTolerance(double tolerance) { params.tolerance = tolerance; }
    double getClusterTolerance() const { return params.tolerance; }
    void setMinClusterSize(int min_cluster_size) { params.min_cluster_size = min_cluster_size; }
    int getMinClusterSize() const { return params.min_cluster_size; }
    void setMaxClusterSize(int max_cluster_size) { params.max_cluster_size = max_cluster_size; }
    int getMaxClusterSize() const { return params.max_cluster_size; }

    void setInputCloud(const PointCloudConstPtr &cloud) { input_ = cloud; }
    const PointCloudConstPtr getInputCloud() const { return input_; }

    // the clusters of input_ (wm_cluster_extract), largest first, each one's indices ascending
    void extract(std::vector<pcl::PointIndices> &clusters);

    // A queue of clouds in one device call (wm_cluster_extract_batch): clusters[k] is what setInputCloud(clouds[k]);
    // extract(...) gives.  The input cloud of the object is not used and not changed.  A null pointer among the
    // clouds, bad parameters or a device error: a LOG_ERROR and `clusters` empty.
    void extractBatch(const std::vector<PointCloudConstPtr> &clouds, std::vector<std::vector<pcl::PointIndices>> &clusters);

 private:
    PointCloudConstPtr input_;
    ClusterExtractionParams params;
    wm_ctx *ctx = nullptr;  // created by the first extract
    int device = 0;
};

}  // namespace wave

#endif  // WAVE_CLUSTEREXTRACTION_HPP
