// wave::ISSKeypoint3D<PointT> on the MI355X back end.
//
// pcl::ISSKeypoint3D without its border estimation: compute() returns the few points of the input cloud worth
// matching -- those whose neighbourhood's scatter matrix has three well separated eigenvalues and whose smallest
// eigenvalue is a local maximum.  One compute() is one C-ABI call, wm_iss_keypoints (include/wavematch.h, which states
// the rule): the neighbour walks, the eigenvalues and the suppression run on the device; the host only copies the
// keypoints out, with all of PointT's fields (pcl::copyPointCloud).
//
// The reference has no such class; this one is shaped like wave::OutlierRemoval<PointT>: the device context is created
// by the first compute(), so construction needs no device; a copy opens a context of its own; bad parameters or a
// device error give a LOG_ERROR and an empty output.  PCL's names are kept.  Differences from PCL's class: the border
// estimation is not built, so setBorderRadius / setNormalRadius with a value > 0 make compute() fail (a LOG_ERROR, an
// empty output) instead of being silently ignored; the two radii have no usable default and must be set; a non-finite
// point is nobody's neighbour and never a keypoint.  libwave_matching.so holds the pcl::PointXYZ instantiation; any
// other point type whose first three floats are x, y, z works after #include <wave/matching/impl/iss_keypoints.hpp>.
#ifndef WAVE_ISSKEYPOINTS_HPP
#define WAVE_ISSKEYPOINTS_HPP

#include <cstddef>
#include <string>
#include <vector>

#include "wave/compat/pcl_filter_min.hpp"
#include "wave/compat/pcl_indices_min.hpp"

struct wm_ctx;  // include/wavematch.h

namespace wave {

struct ISSKeypointParams {
    ISSKeypointParams() {}
    // flat "key: value" YAML file: salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors
    // (libwave_amd/host/iss_keypoints.cpp).  A file that cannot be read logs "Unable to load config" and leaves the
    // defaults, as OutlierRemovalParams does.
    ISSKeypointParams(const std::string &config_path);

    // the defaults are wm_iss_default_params' (PCL's gammas and min_neighbors; the radii must be set)
    double salient_radius = 0;  // metres: the neighbourhood of the scatter matrix
    double non_max_radius = 0;  // metres: the neighbourhood of the non-maximum suppression
    double gamma_21 = 0.975;    // salient iff l2 / l1 < gamma_21 ...
    double gamma_32 = 0.975;    // ... and l3 / l2 < gamma_32
    int min_neighbors = 5;      // neighbours (the point included) both neighbourhoods need
};

namespace detail {
// libwave_amd/host/iss_keypoints.cpp: the non-template part of compute
int issDefaultDevice();
void issRelease(wm_ctx *&ctx);
// the keypoints' indices, ascending; false (after a LOG_ERROR, `out` empty) on bad parameters, a border or normal
// radius > 0 (not built) or a device error.  An empty cloud: true without a device.
bool issIndices(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride, const ISSKeypointParams &params,
                double border_radius, double normal_radius, std::vector<int> &out);
}  // namespace detail

template <typename PointT>
class ISSKeypoint3D {
 public:
    using PointCloud = pcl::PointCloud<PointT>;
    using PointCloudConstPtr = typename PointCloud::ConstPtr;
    using PointIndicesConstPtr = boost::shared_ptr<const pcl::PointIndices>;

    ISSKeypoint3D() : ISSKeypoint3D(ISSKeypointParams()) {}
    explicit ISSKeypoint3D(const ISSKeypointParams &config);  // no device is opened here
    ISSKeypoint3D(const ISSKeypoint3D &other);                // the copy opens a context of its own
    ISSKeypoint3D &operator=(const ISSKeypoint3D &other);
    ~ISSKeypoint3D();

    void setInputCloud(const PointCloudConstPtr &cloud) { input_ = cloud; }
    PointCloudConstPtr getInputCloud() const { return input_; }
    void setSalientRadius(double r) { params.salient_radius = r; }
    void setNonMaxRadius(double r) { params.non_max_radius = r; }
    void setThreshold21(double g) { params.gamma_21 = g; }
    void setThreshold32(double g) { params.gamma_32 = g; }
    void setMinNeighbors(int n) { params.min_neighbors = n; }
    // the border estimation is not built: a value > 0 makes compute() fail
    void setBorderRadius(double r) { border_radius = r; }
    void setNormalRadius(double r) { normal_radius = r; }
    const ISSKeypointParams &getParams() const { return params; }

    // the keypoints of the input cloud, in input order, on the device (wm_iss_keypoints)
    void compute(PointCloud &output);
    // their indices in the input cloud, ascending (of the last compute())
    PointIndicesConstPtr getKeypointsIndices() const { return keypoints_indices_; }

 private:
    ISSKeypointParams params;
    double border_radius = 0, normal_radius = 0;
    PointCloudConstPtr input_;
    boost::shared_ptr<pcl::PointIndices> keypoints_indices_;
    wm_ctx *ctx = nullptr;  // created by the first compute()
    int device = 0;
};

}  // namespace wave

#endif  // WAVE_ISSKEYPOINTS_HPP
