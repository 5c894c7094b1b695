// EuclideanClusterExtraction<PointT>'s member definitions: extract hands the cloud to the device with a stride of
// sizeof(PointT) -- every PCL XYZ point type starts with float x, y, z.
#ifndef WAVE_CLUSTEREXTRACTION_IMPL_HPP
#define WAVE_CLUSTEREXTRACTION_IMPL_HPP

#include "wave/matching/cluster_extraction.hpp"

namespace wave {

template <typename PointT>
EuclideanClusterExtraction<PointT>::EuclideanClusterExtraction() : device{detail::clusterDefaultDevice()} {}

template <typename PointT>
EuclideanClusterExtraction<PointT>::EuclideanClusterExtraction(const ClusterExtractionParams &config)
    : params{config}, device{detail::clusterDefaultDevice()} {}

template <typename PointT>
EuclideanClusterExtraction<PointT>::EuclideanClusterExtraction(const EuclideanClusterExtraction &other)
    : input_{other.input_}, params{other.params}, ctx{nullptr}, device{other.device} {}

template <typename PointT>
EuclideanClusterExtraction<PointT> &EuclideanClusterExtraction<PointT>::operator=(const EuclideanClusterExtraction &other) {
    if (this != &other) {
        input_ = other.input_;
        params = other.params;
        device = other.device;
    }
    return *this;
}

template <typename PointT>
EuclideanClusterExtraction<PointT>::~EuclideanClusterExtraction() {
    detail::clusterRelease(this->ctx);
}

template <typename PointT>
void EuclideanClusterExtraction<PointT>::extract(std::vector<pcl::PointIndices> &clusters) {
    static_assert(sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) % 4 == 0,
                  "EuclideanClusterExtraction: a point type whose first three floats are x, y, z");
    clusters.clear();
    if (!this->input_) return;
    const auto &in = *this->input_;
    if (!detail::clusterExtract(this->ctx, this->device, in.points.empty() ? nullptr : in.points.data(), in.points.size(),
                                sizeof(PointT), this->params, clusters))
        clusters.clear();
}

template <typename PointT>
void EuclideanClusterExtraction<PointT>::extractBatch(const std::vector<PointCloudConstPtr> &clouds,
                                                      std::vector<std::vector<pcl::PointIndices>> &clusters) {
    static_assert(sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) % 4 == 0,
                  "EuclideanClusterExtraction: a point type whose first three floats are x, y, z");
    clusters.clear();
    std::vector<const void *> pts(clouds.size(), nullptr);
    std::vector<size_t> n(clouds.size(), 0);
    for (size_t k = 0; k < clouds.size(); ++k) {
        if (clouds[k]) {
            n[k] = clouds[k]->points.size();
            pts[k] = n[k] ? clouds[k]->points.data() : nullptr;
        } else {
            n[k] = static_cast<size_t>(-1);  // (detail::clusterExtractBatch logs it)
        }
    }
    if (!detail::clusterExtractBatch(this->ctx, this->device, pts, n, sizeof(PointT), this->params, clusters))
        clusters.clear();
}

}  // namespace wave

// PCL_INSTANTIATE_EuclideanClusterExtraction(MyPoint) in one source file of a program precompiles the class for MyPoint
#define PCL_INSTANTIATE_EuclideanClusterExtraction(T) template class wave::EuclideanClusterExtraction<T>;

#endif  // WAVE_CLUSTEREXTRACTION_IMPL_HPP
