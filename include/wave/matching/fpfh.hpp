// wave::FPFHEstimation<PointT> and wave::matchFeatures on the MI355X back end.
//
// pcl::FPFHEstimation's surface with a k-neighbourhood: setInputCloud, setInputNormals, setKSearch, compute; and the
// nearest-descriptor correspondences of pcl::registration::CorrespondenceEstimation<FPFHSignature33, FPFHSignature33>
// (determineCorrespondences, determineReciprocalCorrespondences) as one function.  Together they are what a coarse
// alignment without an initial pose starts from: descriptors of both clouds, matched in descriptor space.  One
// compute() is one C-ABI call, wm_fpfh_estimate, and one matchFeatures() one wm_feature_match (include/wavematch.h,
// "feature descriptors", states the rule bit by bit).
//
// The normals come from one of two sources:
//   setInputNormals(normals, n, stride_bytes)  the caller's array (nx, ny, nz first in each record), not owned: it must
//                                              live until compute() returns and n must be the input cloud's size;
//   setNormalKSearch(k)                        compute() estimates them from each point's k nearest neighbours on the
//                                              device (pcl::NormalEstimation, viewpoint at the origin); the default, 10.
// Differences from PCL's class: there is no radius neighbourhood (setRadiusSearch), no setSearchSurface, no setIndices
// and no setSearchMethod; a point that is not finite or whose normal is (0, 0, 0) gets 33 zeros where PCL writes NaN;
// a cloud with fewer finite points than neighbours asked for is an error.  Shaped like
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
    // flat "key: value" YAML file: feature_k, normal_k (libwave_amd/host/fpfh.cpp).  A file that cannot be read logs
    // "Unable to load config" and leaves the defaults, as ConditionalClusteringParams does.
    FPFHParams(const std::string &config_path);

    int feature_k = 10;  // neighbours of a descriptor, the point itself included, 3 ... 32
    int normal_k = 10;   // neighbours of an estimated normal, 3 ... 32
};

namespace detail {
// libwave_amd/host/fpfh.cpp: the non-template part of compute
int fpfhDefaultDevice();
void fpfhRelease(wm_ctx *&ctx);
// false (after a LOG_ERROR, `out` empty) on bad parameters, missing normals or a device error
bool fpfhCompute(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride, const FPFHParams &params,
                 const float *normals, size_t normals_n, size_t normals_stride, std::vector<pcl::FPFHSignature33> &out);
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

    void setKSearch(int k) { params.feature_k = k; }
    int getKSearch() const { return params.feature_k; }
    void setNormalKSearch(int k) { params.normal_k = k; }
    int getNormalKSearch() const { return params.normal_k; }

    // nullptr: back to estimated normals
    void setInputNormals(const float *normals, size_t n, size_t stride_bytes = 16) {
        normals_ = normals;
        normals_n = n;
        normals_stride = stride_bytes;
    }

    void setInputCloud(const PointCloudConstPtr &cloud) { input_ = cloud; }
    const PointCloudConstPtr getInputCloud() const { return input_; }

    // one descriptor per point of input_, in its order (wm_fpfh_estimate); empty on an error
    void compute(std::vector<pcl::FPFHSignature33> &output);

 private:
    PointCloudConstPtr input_;
    FPFHParams params;
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
