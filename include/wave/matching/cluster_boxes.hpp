// wave::ClusterBoxes<PointT> on the MI355X back end: where each cluster is and how big it is.
//
// The step between EuclideanClusterExtraction and a registration of the clusters of two frames: per cluster the count,
// the axis-aligned box, the centroid, the covariance's eigenvalues and axes and PCL's oriented box -- what
// pcl::MomentOfInertiaEstimation (getMassCenter, getAABB, getOBB, getEigenValues, getEigenVectors), pcl::getMinMax3D
// and pcl::compute3DCentroid give for one cluster at a time.  One compute() is one C-ABI call, wm_cluster_boxes
// (include/wavematch.h, which states the rule and its deviations from PCL), for ALL clusters of the cloud.
//
// The reference has no such class; this one is shaped like wave::EuclideanClusterExtraction<PointT>: the device
// context is created by the first compute(), so construction needs no device; a copy opens a context of its own; a
// bad cluster list (an index outside the cloud) or a device error give a LOG_ERROR and an empty result.
// libwave_matching.so holds the pcl::PointXYZ instantiation; any other point type whose first three floats are x, y, z
// works after #include <wave/matching/impl/cluster_boxes.hpp>.
#ifndef WAVE_CLUSTERBOXES_HPP
#define WAVE_CLUSTERBOXES_HPP

#include <cstddef>
#include <cstdint>
#include <vector>

#include "wave/compat/pcl_indices_min.hpp"

struct wm_ctx;  // include/wavematch.h

namespace wave {

// wm_cluster_box, field for field (128 bytes), with PCL-named accessors.  Those of the moments return false -- PCL's
// is_valid_ -- for a cluster without a finite member or one whose extent the rule cannot hold (flags & RANGE).
struct ClusterBox {
    enum { EMPTY = 1, NONFINITE = 2, RANGE = 4 };  // WM_BOX_*
    uint32_t n = 0;      // finite members
    uint32_t flags = 0;
    float aabb_min[3] = {0, 0, 0}, aabb_max[3] = {0, 0, 0};
    float centroid[3] = {0, 0, 0};
    float eigenvalues[3] = {0, 0, 0};  // descending
    float axes[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // rows: major, middle, minor
    float obb_center[3] = {0, 0, 0};
    float obb_half[3] = {0, 0, 0};
    uint32_t reserved[3] = {0, 0, 0};

    bool hasMoments() const { return n > 0 && !(flags & RANGE); }

    template <typename PointT>
    bool getAABB(PointT &min_point, PointT &max_point) const {
        min_point.x = aabb_min[0], min_point.y = aabb_min[1], min_point.z = aabb_min[2];
        max_point.x = aabb_max[0], max_point.y = aabb_max[1], max_point.z = aabb_max[2];
        return n > 0;
    }
    // PCL's getOBB: the box's corners in its own frame (-half, +half), its centre, and the rotation whose COLUMNS are
    // the major, middle and minor axes
    template <typename PointT>
    bool getOBB(PointT &min_point, PointT &max_point, PointT &position, Eigen::Matrix<float, 3, 3> &rotation) const {
        min_point.x = -obb_half[0], min_point.y = -obb_half[1], min_point.z = -obb_half[2];
        max_point.x = obb_half[0], max_point.y = obb_half[1], max_point.z = obb_half[2];
        position.x = obb_center[0], position.y = obb_center[1], position.z = obb_center[2];
        for (int k = 0; k < 3; ++k)
            for (int i = 0; i < 3; ++i) rotation(i, k) = axes[3 * k + i];
        return hasMoments();
    }
    bool getMassCenter(Eigen::Vector3f &mass_center) const {
        for (int i = 0; i < 3; ++i) mass_center(i) = centroid[i];
        return hasMoments();
    }
    bool getEigenValues(float &major, float &middle, float &minor) const {
        major = eigenvalues[0], middle = eigenvalues[1], minor = eigenvalues[2];
        return hasMoments();
    }
    bool getEigenVectors(Eigen::Vector3f &major, Eigen::Vector3f &middle, Eigen::Vector3f &minor) const {
        for (int i = 0; i < 3; ++i) major(i) = axes[i], middle(i) = axes[3 + i], minor(i) = axes[6 + i];
        return hasMoments();
    }
};
static_assert(sizeof(ClusterBox) == 128, "wave::ClusterBox mirrors wm_cluster_box");

namespace detail {
// libwave_amd/host/cluster_boxes.cpp: the non-template part
int boxesDefaultDevice();
void boxesRelease(wm_ctx *&ctx);
// The boxes of the clusters of a queue of clouds in ONE call of wm_cluster_boxes: pts[k] / n[k] are cloud k's records
// (n[k] == size_t(-1): a null cloud), clusters[k] its clusters; out[k][c] is the box of clusters[k][c].  false (after a
// LOG_ERROR, `out` empty) on a null cloud, a differing number of clouds and cluster lists, an index outside its cloud
// or a device error.
bool boxesCompute(wm_ctx *&ctx, int device, const std::vector<const void *> &pts, const std::vector<size_t> &n,
                  size_t stride, const std::vector<const std::vector<pcl::PointIndices> *> &clusters,
                  std::vector<std::vector<ClusterBox>> &out);
}  // namespace detail

template <typename PointT>
class ClusterBoxes {
 public:
    using PointCloud = pcl::PointCloud<PointT>;
    using PointCloudConstPtr = typename PointCloud::ConstPtr;

    ClusterBoxes();                                  // no device is opened here
    ClusterBoxes(const ClusterBoxes &other);         // the copy opens a context of its own
    ClusterBoxes &operator=(const ClusterBoxes &other);
    ~ClusterBoxes();

    void setInputCloud(const PointCloudConstPtr &cloud) { input_ = cloud; }
    const PointCloudConstPtr getInputCloud() const { return input_; }
    // the clusters of input_, as EuclideanClusterExtraction::extract returns them (any lists of indices will do)
    void setClusters(const std::vector<pcl::PointIndices> &clusters) { clusters_ = clusters; }
    const std::vector<pcl::PointIndices> &getClusters() const { return clusters_; }

    // boxes[c] describes cluster c (wm_cluster_boxes); empty without an input cloud or on an error
    void compute(std::vector<ClusterBox> &boxes);

    // A queue of clouds in one device call: boxes[k] is what setInputCloud(clouds[k]); setClusters(clusters[k]);
    // compute(...) gives.  The object's own cloud and clusters are not used and not changed.  A null pointer among
    // the clouds, clouds.size() != clusters.size() or an error: a LOG_ERROR and `boxes` empty.
    void computeBatch(const std::vector<PointCloudConstPtr> &clouds,
                      const std::vector<std::vector<pcl::PointIndices>> &clusters,
                      std::vector<std::vector<ClusterBox>> &boxes);

 private:
    PointCloudConstPtr input_;
    std::vector<pcl::PointIndices> clusters_;
    wm_ctx *ctx = nullptr;  // created by the first compute
    int device = 0;
};

}  // namespace wave

#endif  // WAVE_CLUSTERBOXES_HPP
