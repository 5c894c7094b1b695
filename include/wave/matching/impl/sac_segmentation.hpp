// SACSegmentation<PointT>'s member definitions: segment hands the cloud to the device with a stride of sizeof(PointT)
// -- every PCL XYZ point type starts with float x, y, z.
#ifndef WAVE_SACSEGMENTATION_IMPL_HPP
#define WAVE_SACSEGMENTATION_IMPL_HPP

#include "wave/matching/sac_segmentation.hpp"

namespace wave {

template <typename PointT>
SACSegmentation<PointT>::SACSegmentation() : device{detail::sacDefaultDevice()} {}

template <typename PointT>
SACSegmentation<PointT>::SACSegmentation(const SACSegmentationParams &config)
    : params{config}, device{detail::sacDefaultDevice()} {}

template <typename PointT>
SACSegmentation<PointT>::SACSegmentation(const SACSegmentation &other)
    : input_{other.input_}, params{other.params}, ctx{nullptr}, device{other.device} {}

template <typename PointT>
SACSegmentation<PointT> &SACSegmentation<PointT>::operator=(const SACSegmentation &other) {
    if (this != &other) {
        input_ = other.input_;
        params = other.params;
        device = other.device;
    }
    return *this;
}

template <typename PointT>
SACSegmentation<PointT>::~SACSegmentation() {
    detail::sacRelease(this->ctx);
}

template <typename PointT>
void SACSegmentation<PointT>::segment(pcl::PointIndices &inliers, pcl::ModelCoefficients &model_coefficients) {
    static_assert(sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) % 4 == 0,
                  "SACSegmentation: a point type whose first three floats are x, y, z");
    inliers.indices.clear();
    model_coefficients.values.clear();
    if (!this->input_) return;
    const auto &in = *this->input_;
    if (!detail::sacSegment(this->ctx, this->device, in.points.empty() ? nullptr : in.points.data(), in.points.size(),
                            sizeof(PointT), this->params, inliers, model_coefficients)) {
        inliers.indices.clear();
        model_coefficients.values.clear();
    }
}

template <typename PointT>
void SACSegmentation<PointT>::segmentBatch(const std::vector<PointCloudConstPtr> &clouds, std::vector<pcl::PointIndices> &inliers,
                                           std::vector<pcl::ModelCoefficients> &coefficients) {
    static_assert(sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) % 4 == 0,
                  "SACSegmentation: a point type whose first three floats are x, y, z");
    const size_t count = clouds.size();
    std::vector<const void *> pts(count, nullptr);
    std::vector<size_t> n(count, 0);
    std::vector<unsigned char> null_cloud(count, 0);  // (not vector<bool>: the flags go over as an array)
    for (size_t k = 0; k < count; ++k) {
        if (!clouds[k]) {
            null_cloud[k] = 1;
            continue;
        }
        n[k] = clouds[k]->points.size();
        if (n[k]) pts[k] = clouds[k]->points.data();
    }
    if (!detail::sacSegmentBatch(this->ctx, this->device, pts.data(), n.data(), null_cloud.data(), count, sizeof(PointT),
                                 this->params, inliers, coefficients)) {
        inliers.assign(count, pcl::PointIndices());
        coefficients.assign(count, pcl::ModelCoefficients());
    }
}

}  // namespace wave

// PCL_INSTANTIATE_SACSegmentation(MyPoint) in one source file of a program precompiles the class for MyPoint
#define PCL_INSTANTIATE_SACSegmentation(T) template class wave::SACSegmentation<T>;

#endif  // WAVE_SACSEGMENTATION_IMPL_HPP
