// ConditionalEuclideanClustering<PointT>'s member definitions: segment hands the cloud to the device with a stride of
// sizeof(PointT) -- every PCL XYZ point type starts with float x, y, z.
#ifndef WAVE_CONDITIONALCLUSTERING_IMPL_HPP
#define WAVE_CONDITIONALCLUSTERING_IMPL_HPP

#include "wave/matching/conditional_clustering.hpp"

namespace wave {

template <typename PointT>
ConditionalEuclideanClustering<PointT>::ConditionalEuclideanClustering() : device{detail::condClusterDefaultDevice()} {}

template <typename PointT>
ConditionalEuclideanClustering<PointT>::ConditionalEuclideanClustering(const ConditionalClusteringParams &config)
    : params{config},
      normal_test{config.max_normal_angle >= 0},
      scalar_test{config.max_scalar_diff >= 0},
      device{detail::condClusterDefaultDevice()} {}

template <typename PointT>
ConditionalEuclideanClustering<PointT>::ConditionalEuclideanClustering(const ConditionalEuclideanClustering &other)
    : input_{other.input_},
      params{other.params},
      normal_test{other.normal_test},
      scalar_test{other.scalar_test},
      attr_{other.attr_},
      attr_n{other.attr_n},
      attr_stride{other.attr_stride},
      ctx{nullptr},
      device{other.device} {}

template <typename PointT>
ConditionalEuclideanClustering<PointT> &ConditionalEuclideanClustering<PointT>::operator=(
  const ConditionalEuclideanClustering &other) {
    if (this != &other) {
        input_ = other.input_;
        params = other.params;
        normal_test = other.normal_test;
        scalar_test = other.scalar_test;
        attr_ = other.attr_;
        attr_n = other.attr_n;
        attr_stride = other.attr_stride;
        device = other.device;
    }
    return *this;
}

template <typename PointT>
ConditionalEuclideanClustering<PointT>::~ConditionalEuclideanClustering() {
    detail::condClusterRelease(this->ctx);
}

template <typename PointT>
void ConditionalEuclideanClustering<PointT>::segment(std::vector<pcl::PointIndices> &clusters) {
    static_assert(sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) % 4 == 0,
                  "ConditionalEuclideanClustering: a point type whose first three floats are x, y, z");
    clusters.clear();
    if (!this->input_) return;
    const auto &in = *this->input_;
    if (!detail::condClusterSegment(this->ctx, this->device, in.points.empty() ? nullptr : in.points.data(),
                                    in.points.size(), sizeof(PointT), this->params, this->normal_test, this->scalar_test,
                                    this->attr_, this->attr_n, this->attr_stride, clusters))
        clusters.clear();
}

}  // namespace wave

// PCL_INSTANTIATE_ConditionalEuclideanClustering(MyPoint) in one source file of a program precompiles the class for MyPoint
#define PCL_INSTANTIATE_ConditionalEuclideanClustering(T) template class wave::ConditionalEuclideanClustering<T>;

#endif  // WAVE_CONDITIONALCLUSTERING_IMPL_HPP
