// wave::CorrespondenceRejectorSampleConsensus<PointT> on the MI355X back end.
//
// pcl::registration::CorrespondenceRejectorSampleConsensus's surface: setInputSource, setInputTarget,
// setInlierThreshold, setMaximumIterations, setRefineModel, getRemainingCorrespondences, getBestTransformation.  RANSAC
// over the correspondences with a rigid transform from three pairs; out come the pairs the best transform brings
// within the threshold, and that transform: the pose a pipeline of descriptors (wave::FPFHEstimation) and matches
// (wave::matchFeatures) ends in.  One getRemainingCorrespondences() is one C-ABI call, wm_corr_ransac
// (include/wavematch.h, "pose from correspondences", states the rule operation by operation and lists the deviations
// from PCL; the samples come from a stream that is a function of the seed, not from rand()).
//
// Extensions: setSeed, setMinSampleDistance (negative, the default: PCL's automatic threshold from the source points
// of the correspondences), setProbability.  setRefineModel(true) is ONE least-squares refit over the model's inliers,
// not PCL's loop with a shrinking threshold.
//
// Without a model -- fewer than three correspondences with finite points, or no sample that passes the sample test --
// the class behaves as PCL's does: the remaining correspondences are the input's and the transformation is the
// identity.  The same after an error (a missing cloud, bad parameters, an index outside its cloud's range is simply not
// a valid correspondence, a device error), behind a LOG_ERROR.
//
// Shaped like wave::FPFHEstimation<PointT>: construction opens no device, the context is created by the first call, a
// copy opens a context of its own.  libwave_matching.so holds the pcl::PointXYZ instantiation; any other point type
// whose first three floats are x, y, z works after #include <wave/matching/impl/correspondence_rejection.hpp>.
#ifndef WAVE_CORRESPONDENCE_REJECTION_HPP
#define WAVE_CORRESPONDENCE_REJECTION_HPP

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "wave/compat/pcl_fpfh_min.hpp"

struct wm_ctx;  // include/wavematch.h

namespace wave {

struct CorrespondenceRejectionParams {
    CorrespondenceRejectionParams() {}
    // flat "key: value" YAML file: inlier_threshold, max_iterations, probability, refine_model, min_sample_distance
    // (libwave_amd/host/correspondence_rejection.cpp).  A file that cannot be read logs "Unable to load config" and
    // leaves the defaults, as FPFHParams does.
    CorrespondenceRejectionParams(const std::string &config_path);

    double inlier_threshold = 0.05;     // PCL's default
    int max_iterations = 1000;          // PCL's default
    double probability = 0.99;
    int refine_model = 0;               // PCL's refine_ = false
    double min_sample_distance = -1.0;  // < 0: from the correspondences' source points
    uint64_t seed = 0;
};

namespace detail {
// libwave_amd/host/correspondence_rejection.cpp: the non-template part
int corrDefaultDevice();
void corrRelease(wm_ctx *&ctx);
// true with `remaining` and T (row-major 4 x 4) written: a model was found.  false: no model, or (after a LOG_ERROR)
// an error; the caller then returns the input and the identity
bool corrRansac(wm_ctx *&ctx, int device, const void *src, size_t n_src, const void *tgt, size_t n_tgt, size_t stride,
                const CorrespondenceRejectionParams &params, const std::vector<pcl::Correspondence> &in,
                std::vector<pcl::Correspondence> &remaining, double T[16]);
}  // namespace detail

template <typename PointT>
class CorrespondenceRejectorSampleConsensus {
 public:
    using PointCloud = pcl::PointCloud<PointT>;
    using PointCloudConstPtr = typename PointCloud::ConstPtr;

    CorrespondenceRejectorSampleConsensus();  // PCL's defaults; no device is opened here
    explicit CorrespondenceRejectorSampleConsensus(const CorrespondenceRejectionParams &config);
    CorrespondenceRejectorSampleConsensus(const CorrespondenceRejectorSampleConsensus &other);  // a context of its own
    CorrespondenceRejectorSampleConsensus &operator=(const CorrespondenceRejectorSampleConsensus &other);
    ~CorrespondenceRejectorSampleConsensus();

    void setInputSource(const PointCloudConstPtr &cloud) { source_ = cloud; }
    void setInputTarget(const PointCloudConstPtr &cloud) { target_ = cloud; }
    const PointCloudConstPtr getInputSource() const { return source_; }
    const PointCloudConstPtr getInputTarget() const { return target_; }

    void setInlierThreshold(double threshold) { params.inlier_threshold = threshold; }
    double getInlierThreshold() const { return params.inlier_threshold; }
    void setMaximumIterations(int max_iterations) { params.max_iterations = max_iterations; }
    int getMaximumIterations() const { return params.max_iterations; }
    void setRefineModel(bool refine) { params.refine_model = refine ? 1 : 0; }
    bool getRefineModel() const { return params.refine_model != 0; }
    void setSeed(uint64_t seed) { params.seed = seed; }
    void setMinSampleDistance(double d) { params.min_sample_distance = d; }
    void setProbability(double p) { params.probability = p; }

    // index_query is a point of the source, index_match a point of the target.  remaining: the correspondences the
    // best transformation keeps, in the input's order; the input itself without a model.
    void getRemainingCorrespondences(const std::vector<pcl::Correspondence> &original,
                                     std::vector<pcl::Correspondence> &remaining);
    // source -> target of the last getRemainingCorrespondences; the identity before it and without a model
    Eigen::Matrix4d getBestTransformation() const { return best_; }

 private:
    PointCloudConstPtr source_, target_;
    CorrespondenceRejectionParams params;
    Eigen::Matrix4d best_ = Eigen::Matrix4d::Identity();
    wm_ctx *ctx = nullptr;  // created by the first call
    int device = 0;
};

}  // namespace wave

#endif  // WAVE_CORRESPONDENCE_REJECTION_HPP
