// wave::FPFHEstimation<PointT> and wave::matchFeatures on the MI355X back end.
//
// pcl::FPFHEstimation's surface: setInputCloud, setInputNormals, setKSearch or setRadiusSearch, compute; and the
// nearest-descriptor correspondences of pcl::registration::CorrespondenceEstimation<FPFHSignature33, FPFHSignature33>
// (determineCorrespondences, determineReciprocalCorrespondences) as one function.  Together they are what a coarse
// alignment without an initial pose starts from: descriptors of both clouds, matched in descriptor space.  One
// compute() is one C-ABI call, wm_fpfh_estimate (k) or wm_fpfh_radius (radius), and one matchFeatures() one
// wm_feature_match (include/wavematch.h, "feature descriptors", states the rules bit by bit).
//
// The neighbourhood is the k nearest points (setKSearch, the default: 10) or a metric radius (setRadiusSearch): a radius
// fixes the physical support whatever the range from the sensor, and it is what PCL's FPFH recipes use, with
// normal_radius < feature_radius.  With a radius compute() hands the input cloud itself to wm_fpfh_radius: nothing is
// set on the context.  A radius and a k both set by the caller is PCL's error, and here a LOG_ERROR and an empty
// result; so is a normal radius beside a normal k, and a feature radius without input normals or a normal radius.
//
// The normals come from one of two sources:
//   setInputNormals(normals, n, stride_bytes)  the caller's array (nx, ny, nz first in each record), not owned: it must
//                                              live until compute() returns and n must be the input cloud's size;
//   setNormalKSearch(k)                        compute() estimates them from each point's k nearest neighbours on the
//                                              device (pcl::NormalEstimation, viewpoint at the origin); the default, 10;
//   setNormalRadiusSearch(r)                   ... from the points within r (the radius form only).
// Differences from PCL's class: no setSearchSurface, no setIndices and no setSearchMethod; a point that is not finite or
// whose normal is (0, 0, 0) gets 33 zeros where PCL writes NaN; with k, a cloud with fewer finite points than
// neighbours asked for is an error; with a radius, a point has at most 8191 neighbours, the weights are r^2 / d^2
// quantised to 2^-20 of the weakest (the factor cancels), a neighbour nearer than r / 256 weighs as one at r / 256, and
// the sums are integers, so that no byte depends on the order of the points (PCL adds in its kd-tree's order).  Shaped like
// wave::ConditionalEuclideanClustering<PointT>: the cloud becomes both clouds of the object's OWN context, created by
// the first compute(), so construction needs no device; a copy opens a context of its own; bad parameters, missing
// normals or a device error give a LOG_ERROR and an empty result.  libwave_matching.so holds the pcl::PointXYZ
// instantiation; any other point type whose first three floats are x, y, z works after
// #include <wave/matching/impl/fpfh.hpp>.
#ifndef WAVE_FPFH_HPP
#define WAVE_FPFH_HPP

#include <cstddef>
#include <string>
#include <vector>

#include "wave/compat/pcl_fpfh_min.hpp"

struct wm_ctx;  // include/wavematch.h

namespace wave {

struct FPFHParams {
    FPFHParams() {}
    // flat "key: value" YAML file: feature_k and normal_k, or feature_radius and normal_radius, or all four
    // (libwave_amd/host/fpfh.cpp).  A file that cannot be read, or that holds neither pair, logs "Unable to load config"
    // and leaves the defaults, as ConditionalClusteringParams does.
    FPFHParams(const std::string &config_path);

    int feature_k = 10;  // neighbours of a descriptor, the point itself included, 3 ... 32
    int normal_k = 10;   // neighbours of an estimated normal, 3 ... 32
    double feature_radius = 0;  // > 0: the radius form (wm_fpfh_radius); the k's are then not read
    double normal_radius = 0;   // the radius of an estimated normal in the radius form
};

namespace detail {
// libwave_amd/host/fpfh.cpp: the non-template part of compute
int fpfhDefaultDevice();
void fpfhRelease(wm_ctx *&ctx);
// false (after a LOG_ERROR, `out` empty) on bad parameters, missing normals or a device error
// k_set / normal_k_set: the caller set that k (an error beside the matching radius)
bool fpfhCompute(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride, const FPFHParams &params, bool k_set,
                 bool normal_k_set, const float *normals, size_t normals_n, size_t normals_stride,
                 std::vector<pcl::FPFHSignature33> &out);
}  // namespace detail

template <typename PointT>
class FPFHEstimation {
 public:
    using PointCloud = pcl::PointCloud<PointT>;
    using PointCloudConstPtr = typename PointCloud::ConstPtr;

    FPFHEstimation();  // both k 10; no device is opened here
    explicit FPFHEstimation(const FPFHParams &config);
    FPFHEstimation(const FPFHEstimation &other);  // the copy opens a context of its own
    FPFHEstimation &operator=(const FPFHEstimation &other);
    ~FPFHEstimation();

    void setKSearch(int k) { params.feature_k = k, k_set = true; }
    int getKSearch() const { return params.feature_k; }
    void setNormalKSearch(int k) { params.normal_k = k, normal_k_set = true; }
    int getNormalKSearch() const { return params.normal_k; }
    // > 0: the neighbourhood is the points within the radius (0: back to k)
    void setRadiusSearch(double radius) { params.feature_radius = radius; }
    double getRadiusSearch() const { return params.feature_radius; }
    void setNormalRadiusSearch(double radius) { params.normal_radius = radius; }
    double getNormalRadiusSearch() const { return params.normal_radius; }

    // nullptr: back to estimated normals
    void setInputNormals(const float *normals, size_t n, size_t stride_bytes = 16) {
        normals_ = normals;
        normals_n = n;
        normals_stride = stride_bytes;
    }

    void setInputCloud(const PointCloudConstPtr &cloud) { input_ = cloud; }
    const PointCloudConstPtr getInputCloud() const { return input_; }

    // one descriptor per point of input_, in its order (wm_fpfh_estimate or wm_fpfh_radius); empty on an error
    void compute(std::vector<pcl::FPFHSignature33> &output);

 private:
    PointCloudConstPtr input_;
    FPFHParams params;
    bool k_set = false, normal_k_set = false;  // setKSearch / setNormalKSearch were called
    const float *normals_ = nullptr;  // not owned
    size_t normals_n = 0, normals_stride = 16;
    wm_ctx *ctx = nullptr;  // created by the first compute
    int device = 0;
};

// For every descriptor of `a` its nearest in `b` (squared distance in float, ties to the lowest index; reciprocal: kept
// only if it is mutual) -> one pcl::Correspondence per matched row of `a`, ascending by index_query, `distance` the
// squared distance.  Rows without a match (all-zero descriptors) are left out, as PCL leaves out what it cannot match.
// The call opens a context on the default device for its duration.  false (after a LOG_ERROR, `out` empty) on an error.
bool matchFeatures(const std::vector<pcl::FPFHSignature33> &a, const std::vector<pcl::FPFHSignature33> &b, bool reciprocal,
                   std::vector<pcl::Correspondence> &out);

}  // namespace wave

#endif  // WAVE_FPFH_HPP
