// wave::GroundSegmentation<PointT> on the MI355X back end.
//
// libwave's Gaussian-process ground filter (after Chen et al., J. Intell. Robot. Syst. 76, 2014) as a pcl::Filter:
// filter() splits the input cloud into ground, obstacle and overhanging points and returns the classes that are
// switched on (by default obstacle and overhanging).  One filter() is one C-ABI call, wm_ground_segment
// (include/wavematch.h): the polar binning, each sector's GP model and the labelling run on the device; the host
// only copies the kept points out.
//
// Interface kept from the reference (wave_matching/include/wave/matching/ground_segmentation.hpp): the class
// template and its base, the constructor from GroundSegmentationParams, setKeepGround / setKeepObstacle /
// setKeepOverhanging, applyFilter, and the SignalPoint struct.  LinCell, AngCell, PolarBinGrid and
// compareSignalPoints held the CPU algorithm's state and are not provided.  Differences: each
// filter() classifies its input afresh (the reference's index vectors grow from call to call); the device context
// is created by the first filter(), so construction needs no device; bad parameters give a LOG_ERROR and an empty
// output.  libwave_matching.so holds the pcl::PointXYZ instantiation; any other point type whose first three
// floats are x, y, z works after #include <wave/matching/impl/ground_segmentation.hpp>.
//
// Addition (the reference has no such member, it filters one scan per call): filterBatch() classifies a queue of
// scans in ONE device call (wm_ground_segment_batch) and gives per scan what setInputCloud + filter would.
#ifndef WAVE_GROUNDSEGMENTATION_HPP
#define WAVE_GROUNDSEGMENTATION_HPP

#include <cstddef>
#include <vector>

#include "wave/compat/pcl_filter_min.hpp"
#include "wave/matching/ground_segmentation_params.hpp"
#include "wave/utils/math.hpp"

struct wm_ctx;  // include/wavematch.h

namespace wave {

// a cell's (range, height) sample of a sector's ground profile in the reference's algorithm; kept for source
// compatibility, the device holds its own form of it
struct SignalPoint {
    double range;
    double height;
    int index;
    bool is_ground;
};

namespace detail {
// libwave_amd/host/ground_segmentation.cpp: the non-template part of applyFilter
int groundDefaultDevice();
void groundRelease(wm_ctx *&ctx);
// the kept points' indices in output order; false (after a LOG_ERROR) on bad parameters or a device error
bool groundSegmentIndices(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride,
                          const GroundSegmentationParams &params, bool keep_ground, bool keep_obs, bool keep_drv,
                          std::vector<int> &out);
// the same for `count` scans in one device call (wm_ground_segment_batch): out[k] = scan k's kept indices
void groundLogNullScan(size_t k);  // LOG_ERROR: entry k of a batch is null
bool groundSegmentIndicesBatch(wm_ctx *&ctx, int device, const void *const *pts, const size_t *n, size_t count,
                               size_t stride, const GroundSegmentationParams &params, bool keep_ground, bool keep_obs,
                               bool keep_drv, std::vector<std::vector<int>> &out);
}  // namespace detail

template <typename PointT>
class GroundSegmentation : public pcl::Filter<PointT> {
 public:
    using PointCloud = typename pcl::Filter<PointT>::PointCloud;
    using PointCloudConstPtr = typename pcl::Filter<PointT>::PointCloudConstPtr;

    // which of the three classes filter() returns, in this order: ground, obstacle, overhanging
    // (defaults: false, true, true)
    void setKeepGround(bool v) { keep_ground = v; }
    void setKeepObstacle(bool v) { keep_obs = v; }
    void setKeepOverhanging(bool v) { keep_drv = v; }

    explicit GroundSegmentation(const GroundSegmentationParams &config);  // no device is opened here
    GroundSegmentation(const GroundSegmentation &other);                  // the copy opens a context of its own
    GroundSegmentation &operator=(const GroundSegmentation &other);
    ~GroundSegmentation() override;

    // classifies input_ on the device (wm_ground_segment) and copies the kept points to `output`
    void applyFilter(PointCloud &output) override;

    // Not in the reference.  outputs[k] = what setInputCloud(inputs[k]); filter(outputs[k]); gives -- the same points
    // in the same order with all of PointT's fields, the same width / height / is_dense -- for the whole queue in one
    // device call.  The keep flags apply to every scan; a null entry gives an empty cloud and a LOG_ERROR; the
    // filter's own input cloud is left alone.
    void filterBatch(const std::vector<PointCloudConstPtr> &inputs, std::vector<PointCloud> &outputs);

 private:
    GroundSegmentationParams params;
    bool keep_ground = false;
    bool keep_obs = true;
    bool keep_drv = true;
    wm_ctx *ctx = nullptr;  // created by the first applyFilter
    int device = 0;
};

}  // namespace wave

#endif  // WAVE_GROUNDSEGMENTATION_HPP
