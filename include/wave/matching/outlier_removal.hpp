// wave::OutlierRemoval<PointT> on the MI355X back end.
//
// pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval as one pcl::Filter: filter() removes isolated returns
// (dust, rain, mixed pixels, points behind glass) from the input cloud.  One filter() is one C-ABI call,
// wm_outlier_filter (include/wavematch.h, which states the two filters' rules): the neighbour searches, the
// statistics and the kept list are formed on the device; the host only copies the kept points out, with all of
// PointT's fields (pcl::copyPointCloud).
//
// The reference has no such class (its pipelines call PCL's two filters); this one is shaped like
// wave::GroundSegmentation<PointT>: the device context is created by the first filter(), so construction needs no
// device; a copy opens a context of its own; bad parameters or a device error give a LOG_ERROR and an empty output.
// Differences from PCL's filters: mean_k is 1 ... 31; a non-finite point is nobody's neighbour and is never returned,
// with either setting of setNegative (PCL keeps it).  libwave_matching.so holds the pcl::PointXYZ instantiation;
// any other point type whose first three floats are x, y, z works after
// #include <wave/matching/impl/outlier_removal.hpp>.
//
// filterBatch() filters a queue of scans in ONE C-ABI call, wm_outlier_filter_batch: every output equals what filter()
// gives for that scan alone, and the per-call cost (the packing, the grid, the fetches and the wait) is paid once.
#ifndef WAVE_OUTLIERREMOVAL_HPP
#define WAVE_OUTLIERREMOVAL_HPP

#include <cstddef>
#include <string>
#include <vector>

#include "wave/compat/pcl_filter_min.hpp"

struct wm_ctx;  // include/wavematch.h

namespace wave {

struct OutlierRemovalParams {
    enum Method { Statistical = 0, Radius = 1 };

    OutlierRemovalParams() {}
    // flat "key: value" YAML file: method (0 statistical, 1 radius), mean_k, stddev_mult, radius, min_neighbors,
    // negative (libwave_amd/host/outlier_removal.cpp).  A file that cannot be read logs "Unable to load config" and
    // leaves the defaults, as GroundSegmentationParams does.
    OutlierRemovalParams(const std::string &config_path);

    // the defaults are PCL's (wm_outlier_default_params)
    int method = Statistical;
    int mean_k = 1;          // statistical: neighbours per point (1 ... 31)
    double stddev_mult = 0;  // statistical: outlier beyond mean + stddev_mult * stddev of the mean distances
    double radius = 0;       // radius: metres (must be set > 0 for the radius filter)
    int min_neighbors = 1;   // radius: inlier with at least this many other points closer than `radius`
    int negative = 0;        // != 0: filter() returns the outliers
};

namespace detail {
// libwave_amd/host/outlier_removal.cpp: the non-template part of applyFilter
int outlierDefaultDevice();
void outlierRelease(wm_ctx *&ctx);
// the kept points' indices, ascending; false (after a LOG_ERROR) on bad parameters or a device error
bool outlierIndices(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride,
                    const OutlierRemovalParams &params, std::vector<int> &out);
// the same for `count` clouds in one wm_outlier_filter_batch call: out[k] = cloud k's kept indices.  A null cloud
// (null_cloud[k]) is logged and gives an empty list, as a cloud that is not converged does; false (after a LOG_ERROR,
// every list empty) on bad parameters or a device error
bool outlierIndicesBatch(wm_ctx *&ctx, int device, const void *const *pts, const size_t *n, const unsigned char *null_cloud,
                         size_t count, size_t stride, const OutlierRemovalParams &params,
                         std::vector<std::vector<int>> &out);
}  // namespace detail

template <typename PointT>
class OutlierRemoval : public pcl::Filter<PointT> {
 public:
    using PointCloud = typename pcl::Filter<PointT>::PointCloud;
    using PointCloudConstPtr = typename pcl::Filter<PointT>::PointCloudConstPtr;

    explicit OutlierRemoval(const OutlierRemovalParams &config);  // no device is opened here
    OutlierRemoval(const OutlierRemoval &other);                  // the copy opens a context of its own
    OutlierRemoval &operator=(const OutlierRemoval &other);
    ~OutlierRemoval() override;

    void setNegative(bool v) { params.negative = v ? 1 : 0; }  // true: filter() returns what it would remove
    bool getNegative() const { return params.negative != 0; }

    // filters input_ on the device (wm_outlier_filter) and copies the kept points to `output`, in input order
    void applyFilter(PointCloud &output) override;

    // filter() for every cloud of `inputs` in one device call (wm_outlier_filter_batch): outputs[k] equals what
    // setInputCloud(inputs[k]) + filter() gives.  A null cloud is logged and gives an empty output, as a cloud with
    // fewer than mean_k + 1 finite points does; bad parameters or a device error log and give empty outputs.
    void filterBatch(const std::vector<PointCloudConstPtr> &inputs, std::vector<PointCloud> &outputs);

 private:
    OutlierRemovalParams params;
    wm_ctx *ctx = nullptr;  // created by the first applyFilter
    int device = 0;
};

}  // namespace wave

#endif  // WAVE_OUTLIERREMOVAL_HPP
