// wave::SACSegmentation<PointT> on the MI355X back end.
//
// pcl::SACSegmentation's surface for a plane model and RANSAC: setModelType / setMethodType / setDistanceThreshold /
// setMaxIterations / setProbability / setOptimizeCoefficients / setAxis / setEpsAngle, setInputCloud,
// segment(pcl::PointIndices &, pcl::ModelCoefficients &).  It finds the road, a wall or a table top -- what a caller
// peels off before clustering.  One segment() is one C-ABI call, wm_sac_segment (include/wavematch.h, which states the
// rule): hypotheses, counts, refit sums and the inlier list are formed on the device; the host walks PCL's loop.
// segmentBatch() segments a queue of clouds in ONE C-ABI call, wm_sac_segment_batch: every element equals what
// segment() gives for that cloud alone.
//
// The reference has no such class (its pipelines call PCL's); this one is shaped like
// wave::EuclideanClusterExtraction<PointT>: the device context is created by the first segment(), so construction needs
// no device; a copy opens a context of its own; bad parameters, a cloud without a model or a device error give a
// LOG_ERROR and both outputs empty.  Differences from PCL's class: the samples come from a counter-based stream with a
// seed (setSeed; PCL draws from rand()), so two runs give the same plane; only the three plane models and SAC_RANSAC
// are built; there is no setIndices, setInputNormals or setSamplesMaxDist.  libwave_matching.so holds the
// pcl::PointXYZ instantiation; any other point type whose first three floats are x, y, z works after
// #include <wave/matching/impl/sac_segmentation.hpp>.
#ifndef WAVE_SACSEGMENTATION_HPP
#define WAVE_SACSEGMENTATION_HPP

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "wave/compat/pcl_model_coefficients_min.hpp"

struct wm_ctx;  // include/wavematch.h

namespace wave {

struct SACSegmentationParams {
    SACSegmentationParams() {}
    // flat "key: value" YAML file: model_type (pcl::SACMODEL_*), distance_threshold, max_iterations, probability,
    // optimize_coefficients, axis_x, axis_y, axis_z, eps_angle, seed (libwave_amd/host/sac_segmentation.cpp).  A file
    // that cannot be read logs "Unable to load config" and leaves the defaults, as ClusterExtractionParams does.
    SACSegmentationParams(const std::string &config_path);

    // the defaults are PCL's (wm_sac_default_params)
    int model_type = pcl::SACMODEL_PLANE;  // or SACMODEL_PERPENDICULAR_PLANE / SACMODEL_PARALLEL_PLANE
    int method_type = pcl::SAC_RANSAC;     // the only one
    double distance_threshold = 0;         // metres (must be set > 0)
    int max_iterations = 50;
    double probability = 0.99;
    bool optimize_coefficients = true;
    double axis[3] = {0, 0, 0};            // the two axis models
    double eps_angle = 0;                  // radians
    uint64_t seed = 0;
};

namespace detail {
// libwave_amd/host/sac_segmentation.cpp: the non-template part of segment
int sacDefaultDevice();
void sacRelease(wm_ctx *&ctx);
// false (after a LOG_ERROR, both outputs empty) on bad parameters, a cloud without a model or a device error
bool sacSegment(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride, const SACSegmentationParams &params,
                pcl::PointIndices &inliers, pcl::ModelCoefficients &coefficients);
// `count` clouds in one wm_sac_segment_batch call; null_cloud[k] != 0: cloud k was a null pointer (logged, treated as
// empty).  A cloud without a model gets empty indices and empty values (logged); false: nothing could be run (after a
// LOG_ERROR, every output empty).  No cloud of three points or more: true without a device.
bool sacSegmentBatch(wm_ctx *&ctx, int device, const void *const *pts, const size_t *n, const unsigned char *null_cloud,
                     size_t count, size_t stride, const SACSegmentationParams &params, std::vector<pcl::PointIndices> &inliers,
                     std::vector<pcl::ModelCoefficients> &coefficients);
}  // namespace detail

template <typename PointT>
class SACSegmentation {
 public:
    using PointCloud = pcl::PointCloud<PointT>;
    using PointCloudConstPtr = typename PointCloud::ConstPtr;

    SACSegmentation();                                        // PCL's defaults; no device is opened here
    explicit SACSegmentation(const SACSegmentationParams &config);
    SACSegmentation(const SACSegmentation &other);            // the copy opens a context of its own
    SACSegmentation &operator=(const SACSegmentation &other);
    ~SACSegmentation();

    void setModelType(int model) { params.model_type = model; }
    int getModelType() const { return params.model_type; }
    void setMethodType(int method) { params.method_type = method; }
    int getMethodType() const { return params.method_type; }
    void setDistanceThreshold(double threshold) { params.distance_threshold = threshold; }
    double getDistanceThreshold() const { return params.distance_threshold; }
    void setMaxIterations(int max_iterations) { params.max_iterations = max_iterations; }
    int getMaxIterations() const { return params.max_iterations; }
    void setProbability(double probability) { params.probability = probability; }
    double getProbability() const { return params.probability; }
    void setOptimizeCoefficients(bool optimize) { params.optimize_coefficients = optimize; }
    bool getOptimizeCoefficients() const { return params.optimize_coefficients; }
    void setAxis(double x, double y, double z) {
        params.axis[0] = x;
        params.axis[1] = y;
        params.axis[2] = z;
    }
    template <class Vec3>
    void setAxis(const Vec3 &ax) {  // (an Eigen::Vector3f, as PCL's)
        setAxis(ax[0], ax[1], ax[2]);
    }
    const double *getAxis() const { return params.axis; }
    void setEpsAngle(double eps_angle) { params.eps_angle = eps_angle; }
    double getEpsAngle() const { return params.eps_angle; }
    void setSeed(uint64_t seed) { params.seed = seed; }
    uint64_t getSeed() const { return params.seed; }

    void setInputCloud(const PointCloudConstPtr &cloud) { input_ = cloud; }
    const PointCloudConstPtr getInputCloud() const { return input_; }

    // the plane of input_ (wm_sac_segment): its inliers ascending, its four coefficients a b c d
    void segment(pcl::PointIndices &inliers, pcl::ModelCoefficients &model_coefficients);

    // Addition (PCL segments one cloud per call): a queue of clouds in ONE C-ABI call, wm_sac_segment_batch.  Element k
    // of both outputs equals what segment() gives for clouds[k] alone; a cloud without a model gets empty indices and
    // empty values; a null cloud is logged and treated as empty; empty vectors are legal.  The input cloud set by
    // setInputCloud is not used.
    void segmentBatch(const std::vector<PointCloudConstPtr> &clouds, std::vector<pcl::PointIndices> &inliers,
                      std::vector<pcl::ModelCoefficients> &coefficients);

 private:
    PointCloudConstPtr input_;
    SACSegmentationParams params;
    wm_ctx *ctx = nullptr;  // created by the first segment
    int device = 0;
};

}  // namespace wave

#endif  // WAVE_SACSEGMENTATION_HPP
