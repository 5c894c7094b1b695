// ClusterBoxes<PointT>'s member definitions: compute hands the cloud to the device with a stride of sizeof(PointT) --
// every PCL XYZ point type starts with float x, y, z.
#ifndef WAVE_CLUSTERBOXES_IMPL_HPP
#define WAVE_CLUSTERBOXES_IMPL_HPP

#include "wave/matching/cluster_boxes.hpp"

namespace wave {

template <typename PointT>
ClusterBoxes<PointT>::ClusterBoxes() : device{detail::boxesDefaultDevice()} {}

template <typename PointT>
ClusterBoxes<PointT>::ClusterBoxes(const ClusterBoxes &other)
    : input_{other.input_}, clusters_{other.clusters_}, ctx{nullptr}, device{other.device} {}

template <typename PointT>
ClusterBoxes<PointT> &ClusterBoxes<PointT>::operator=(const ClusterBoxes &other) {
    if (this != &other) {
        input_ = other.input_;
        clusters_ = other.clusters_;
        device = other.device;
    }
    return *this;
}

template <typename PointT>
ClusterBoxes<PointT>::~ClusterBoxes() {
    detail::boxesRelease(this->ctx);
}

template <typename PointT>
void ClusterBoxes<PointT>::compute(std::vector<ClusterBox> &boxes) {
    static_assert(sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) % 4 == 0,
                  "ClusterBoxes: a point type whose first three floats are x, y, z");
    boxes.clear();
    if (!this->input_) return;
    const auto &in = *this->input_;
    std::vector<std::vector<ClusterBox>> out;
    if (detail::boxesCompute(this->ctx, this->device, {in.points.empty() ? nullptr : in.points.data()}, {in.points.size()},
                             sizeof(PointT), {&this->clusters_}, out) &&
        out.size() == 1)
        boxes.swap(out[0]);
}

template <typename PointT>
void ClusterBoxes<PointT>::computeBatch(const std::vector<PointCloudConstPtr> &clouds,
                                        const std::vector<std::vector<pcl::PointIndices>> &clusters,
                                        std::vector<std::vector<ClusterBox>> &boxes) {
    static_assert(sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) % 4 == 0,
                  "ClusterBoxes: a point type whose first three floats are x, y, z");
    boxes.clear();
    std::vector<const void *> pts(clouds.size(), nullptr);
    std::vector<size_t> n(clouds.size(), 0);
    std::vector<const std::vector<pcl::PointIndices> *> lists(clusters.size(), nullptr);
    for (size_t k = 0; k < clouds.size(); ++k) {
        if (clouds[k]) {
            n[k] = clouds[k]->points.size();
            pts[k] = n[k] ? clouds[k]->points.data() : nullptr;
        } else {
            n[k] = static_cast<size_t>(-1);  // (detail::boxesCompute logs it)
        }
    }
    for (size_t k = 0; k < clusters.size(); ++k) lists[k] = &clusters[k];
    if (!detail::boxesCompute(this->ctx, this->device, pts, n, sizeof(PointT), lists, boxes)) boxes.clear();
}

}  // namespace wave

// PCL_INSTANTIATE_ClusterBoxes(MyPoint) in one source file of a program precompiles the class for MyPoint
#define PCL_INSTANTIATE_ClusterBoxes(T) template class wave::ClusterBoxes<T>;

#endif  // WAVE_CLUSTERBOXES_IMPL_HPP
