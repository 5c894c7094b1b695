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

template <typename PointT>
void OutlierRemoval<PointT>::filterBatch(const std::vector<PointCloudConstPtr> &inputs, std::vector<PointCloud> &outputs) {
    static_assert(sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) % 4 == 0,
                  "OutlierRemoval: a point type whose first three floats are x, y, z");
    const PointCloud none;
    const size_t count = inputs.size();
    std::vector<const void *> pts(count, nullptr);
    std::vector<size_t> n(count, 0);
    std::vector<unsigned char> null_cloud(count, 0);  // (not vector<bool>: the flags go over as an array)
    for (size_t k = 0; k < count; ++k) {
        if (!inputs[k]) {
            null_cloud[k] = 1;
            continue;
        }
        n[k] = inputs[k]->points.size();
        if (n[k]) pts[k] = inputs[k]->points.data();
    }
    std::vector<std::vector<int>> kept;
    if (!detail::outlierIndicesBatch(this->ctx, this->device, pts.data(), n.data(), null_cloud.data(), count,
                                     sizeof(PointT), this->params, kept))
        kept.assign(count, std::vector<int>());
    std::vector<PointCloud> result(count);  // (formed aside: `outputs` may hold the inputs' clouds)
    for (size_t k = 0; k < count; ++k) pcl::copyPointCloud(inputs[k] ? *inputs[k] : none, kept[k], result[k]);
    outputs.swap(result);
}

}  // namespace wave

// PCL_INSTANTIATE_OutlierRemoval(MyPoint) in one source file of a program precompiles the filter for MyPoint
#define PCL_INSTANTIATE_OutlierRemoval(T) template class wave::OutlierRemoval<T>;

#endif  // WAVE_OUTLIERREMOVAL_IMPL_HPP
