// OutlierRemoval<PointT>'s member definitions: applyFilter hands the cloud to the device with a stride of
// sizeof(PointT) -- every PCL XYZ point type starts with float x, y, z -- and copies the kept points out.
#ifndef WAVE_OUTLIERREMOVAL_IMPL_HPP
#define WAVE_OUTLIERREMOVAL_IMPL_HPP

#include "wave/matching/outlier_removal.hpp"

namespace wave {

template <typename PointT>
OutlierRemoval<PointT>::OutlierRemoval(const OutlierRemovalParams &config)
    : params{config}, device{detail::outlierDefaultDevice()} {}

template <typename PointT>
OutlierRemoval<PointT>::OutlierRemoval(const OutlierRemoval &other)
    : pcl::Filter<PointT>(other), params{other.params}, ctx{nullptr}, device{other.device} {}

template <typename PointT>
OutlierRemoval<PointT> &OutlierRemoval<PointT>::operator=(const OutlierRemoval &other) {
    if (this != &other) {
        pcl::Filter<PointT>::operator=(other);
        params = other.params;
        device = other.device;
    }
    return *this;
}

template <typename PointT>
OutlierRemoval<PointT>::~OutlierRemoval() {
    detail::outlierRelease(this->ctx);
}

template <typename PointT>
void OutlierRemoval<PointT>::applyFilter(PointCloud &output) {
    static_assert(sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) % 4 == 0,
                  "OutlierRemoval: a point type whose first three floats are x, y, z");
    std::vector<int> out_indices;
    const auto &in = *this->input_;
    if (!detail::outlierIndices(this->ctx, this->device, in.points.empty() ? nullptr : in.points.data(),
                                in.points.size(), sizeof(PointT), this->params, out_indices))
        out_indices.clear();
    pcl::copyPointCloud(in, out_indices, output);
}

}  // namespace wave

// PCL_INSTANTIATE_OutlierRemoval(MyPoint) in one source file of a program precompiles the filter for MyPoint
#define PCL_INSTANTIATE_OutlierRemoval(T) template class wave::OutlierRemoval<T>;

#endif  // WAVE_OUTLIERREMOVAL_IMPL_HPP
