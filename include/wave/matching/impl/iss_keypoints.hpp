// ISSKeypoint3D<PointT>'s member definitions: compute hands the cloud to the device with a stride of sizeof(PointT)
// -- every PCL XYZ point type starts with float x, y, z -- and copies the keypoints out.
#ifndef WAVE_ISSKEYPOINTS_IMPL_HPP
#define WAVE_ISSKEYPOINTS_IMPL_HPP

#include "wave/matching/iss_keypoints.hpp"

namespace wave {

template <typename PointT>
ISSKeypoint3D<PointT>::ISSKeypoint3D(const ISSKeypointParams &config)
    : params{config}, keypoints_indices_{boost::make_shared<pcl::PointIndices>()}, device{detail::issDefaultDevice()} {}

template <typename PointT>
ISSKeypoint3D<PointT>::ISSKeypoint3D(const ISSKeypoint3D &other)
    : params{other.params},
      border_radius{other.border_radius},
      normal_radius{other.normal_radius},
      input_{other.input_},
      keypoints_indices_{boost::make_shared<pcl::PointIndices>(*other.keypoints_indices_)},
      ctx{nullptr},
      device{other.device} {}

template <typename PointT>
ISSKeypoint3D<PointT> &ISSKeypoint3D<PointT>::operator=(const ISSKeypoint3D &other) {
    if (this != &other) {
        params = other.params;
        border_radius = other.border_radius;
        normal_radius = other.normal_radius;
        input_ = other.input_;
        keypoints_indices_ = boost::make_shared<pcl::PointIndices>(*other.keypoints_indices_);
        device = other.device;
    }
    return *this;
}

template <typename PointT>
ISSKeypoint3D<PointT>::~ISSKeypoint3D() {
    detail::issRelease(this->ctx);
}

template <typename PointT>
void ISSKeypoint3D<PointT>::compute(PointCloud &output) {
    static_assert(sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) % 4 == 0,
                  "ISSKeypoint3D: a point type whose first three floats are x, y, z");
    auto found = boost::make_shared<pcl::PointIndices>();
    const PointCloud none;
    const PointCloud &in = input_ ? *input_ : none;
    if (!detail::issIndices(this->ctx, this->device, in.points.empty() ? nullptr : in.points.data(), in.points.size(),
                            sizeof(PointT), this->params, this->border_radius, this->normal_radius, found->indices))
        found->indices.clear();
    keypoints_indices_ = found;
    PointCloud result;  // (formed aside: `output` may be the input)
    pcl::copyPointCloud(in, found->indices, result);
    output = result;
}

}  // namespace wave

// PCL_INSTANTIATE_ISSKeypoint3D(MyPoint) in one source file of a program precompiles the detector for MyPoint
#define PCL_INSTANTIATE_ISSKeypoint3D(T) template class wave::ISSKeypoint3D<T>;

#endif  // WAVE_ISSKEYPOINTS_IMPL_HPP
