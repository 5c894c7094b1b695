// GroundSegmentation<PointT>'s member definitions (wave_matching/include/wave/matching/impl/
// ground_segmentation.hpp:10-381): applyFilter hands the cloud to the device with a stride of sizeof(PointT) --
// every PCL XYZ point type starts with float x, y, z -- and copies the kept points out (pcl::copyPointCloud, :380).
#ifndef WAVE_GROUNDSEGMENTATION_IMPL_HPP
#define WAVE_GROUNDSEGMENTATION_IMPL_HPP

#include "wave/matching/ground_segmentation.hpp"

namespace wave {

template <typename PointT>
GroundSegmentation<PointT>::GroundSegmentation(const GroundSegmentationParams &config)
    : params{config}, device{detail::groundDefaultDevice()} {}

template <typename PointT>
GroundSegmentation<PointT>::GroundSegmentation(const GroundSegmentation &other)
    : pcl::Filter<PointT>(other),
      params{other.params},
      keep_ground{other.keep_ground},
      keep_obs{other.keep_obs},
      keep_drv{other.keep_drv},
      ctx{nullptr},
      device{other.device} {}

template <typename PointT>
GroundSegmentation<PointT> &GroundSegmentation<PointT>::operator=(const GroundSegmentation &other) {
    if (this != &other) {
        pcl::Filter<PointT>::operator=(other);
        params = other.params;
        keep_ground = other.keep_ground;
        keep_obs = other.keep_obs;
        keep_drv = other.keep_drv;
        device = other.device;
    }
    return *this;
}

template <typename PointT>
GroundSegmentation<PointT>::~GroundSegmentation() {
    detail::groundRelease(this->ctx);
}

template <typename PointT>
void GroundSegmentation<PointT>::applyFilter(PointCloud &output) {
    static_assert(sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) % 4 == 0,
                  "GroundSegmentation: a point type whose first three floats are x, y, z");
    std::vector<int> out_indices;
    const auto &in = *this->input_;
    if (!detail::groundSegmentIndices(this->ctx, this->device, in.points.empty() ? nullptr : in.points.data(),
                                      in.points.size(), sizeof(PointT), this->params, this->keep_ground,
                                      this->keep_obs, this->keep_drv, out_indices))
        out_indices.clear();
    pcl::copyPointCloud(in, out_indices, output);
}

template <typename PointT>
void GroundSegmentation<PointT>::filterBatch(const std::vector<PointCloudConstPtr> &inputs,
                                             std::vector<PointCloud> &outputs) {
    static_assert(sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) % 4 == 0,
                  "GroundSegmentation: a point type whose first three floats are x, y, z");
    const PointCloud none;
    std::vector<const void *> pts(inputs.size(), nullptr);
    std::vector<size_t> n(inputs.size(), 0);
    for (size_t k = 0; k < inputs.size(); ++k) {
        if (!inputs[k]) {
            detail::groundLogNullScan(k);
            continue;
        }
        n[k] = inputs[k]->points.size();
        if (n[k]) pts[k] = inputs[k]->points.data();
    }
    std::vector<std::vector<int>> kept;
    if (!detail::groundSegmentIndicesBatch(this->ctx, this->device, pts.data(), n.data(), inputs.size(),
                                           sizeof(PointT), this->params, this->keep_ground, this->keep_obs,
                                           this->keep_drv, kept))
        kept.assign(inputs.size(), std::vector<int>());
    std::vector<PointCloud> result(inputs.size());  // (formed aside: `outputs` may hold the inputs' clouds)
    for (size_t k = 0; k < inputs.size(); ++k) pcl::copyPointCloud(inputs[k] ? *inputs[k] : none, kept[k], result[k]);
    outputs.swap(result);
}

}  // namespace wave

// the reference's impl header also defines this macro: PCL_INSTANTIATE_GroundSegmentation(MyPoint) in one source file
// of a program precompiles the filter for MyPoint
#define PCL_INSTANTIATE_GroundSegmentation(T) template class wave::GroundSegmentation<T>;

#endif  // WAVE_GROUNDSEGMENTATION_IMPL_HPP
