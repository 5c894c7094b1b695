// FPFHEstimation<PointT>'s member definitions: compute hands the cloud to the device with a stride of sizeof(PointT) --
// every PCL XYZ point type starts with float x, y, z.
#ifndef WAVE_FPFH_IMPL_HPP
#define WAVE_FPFH_IMPL_HPP

#include "wave/matching/fpfh.hpp"

namespace wave {

template <typename PointT>
FPFHEstimation<PointT>::FPFHEstimation() : device{detail::fpfhDefaultDevice()} {}

template <typename PointT>
FPFHEstimation<PointT>::FPFHEstimation(const FPFHParams &config) : params{config}, device{detail::fpfhDefaultDevice()} {}

template <typename PointT>
FPFHEstimation<PointT>::FPFHEstimation(const FPFHEstimation &other)
    : input_{other.input_},
      params{other.params},
      k_set{other.k_set},
      normal_k_set{other.normal_k_set},
      normals_{other.normals_},
      normals_n{other.normals_n},
      normals_stride{other.normals_stride},
      ctx{nullptr},
      device{other.device} {}

template <typename PointT>
FPFHEstimation<PointT> &FPFHEstimation<PointT>::operator=(const FPFHEstimation &other) {
    if (this != &other) {
        input_ = other.input_;
        params = other.params;
        k_set = other.k_set;
        normal_k_set = other.normal_k_set;
        normals_ = other.normals_;
        normals_n = other.normals_n;
        normals_stride = other.normals_stride;
        device = other.device;
    }
    return *this;
}

template <typename PointT>
FPFHEstimation<PointT>::~FPFHEstimation() {
    detail::fpfhRelease(this->ctx);
}

template <typename PointT>
void FPFHEstimation<PointT>::compute(std::vector<pcl::FPFHSignature33> &output) {
    static_assert(sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) % 4 == 0,
                  "FPFHEstimation: a point type whose first three floats are x, y, z");
    output.clear();
    if (!this->input_ || this->input_->points.empty()) return;
    const auto &in = *this->input_;
    if (!detail::fpfhCompute(this->ctx, this->device, in.points.data(), in.points.size(), sizeof(PointT), this->params,
                             this->k_set, this->normal_k_set, this->normals_, this->normals_n, this->normals_stride, output))
        output.clear();
}

}  // namespace wave

// PCL_INSTANTIATE_FPFHEstimation(MyPoint) in one source file of a program precompiles the class for MyPoint
#define PCL_INSTANTIATE_FPFHEstimation(T) template class wave::FPFHEstimation<T>;

#endif  // WAVE_FPFH_IMPL_HPP
