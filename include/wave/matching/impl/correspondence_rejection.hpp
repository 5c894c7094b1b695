// CorrespondenceRejectorSampleConsensus<PointT>'s member definitions: the clouds go to the device with a stride of
// sizeof(PointT) -- every PCL XYZ point type starts with float x, y, z.
#ifndef WAVE_CORRESPONDENCE_REJECTION_IMPL_HPP
#define WAVE_CORRESPONDENCE_REJECTION_IMPL_HPP

#include "wave/matching/correspondence_rejection.hpp"

namespace wave {

template <typename PointT>
CorrespondenceRejectorSampleConsensus<PointT>::CorrespondenceRejectorSampleConsensus() : device{detail::corrDefaultDevice()} {}

template <typename PointT>
CorrespondenceRejectorSampleConsensus<PointT>::CorrespondenceRejectorSampleConsensus(const CorrespondenceRejectionParams &config)
    : params{config}, device{detail::corrDefaultDevice()} {}

template <typename PointT>
CorrespondenceRejectorSampleConsensus<PointT>::CorrespondenceRejectorSampleConsensus(const CorrespondenceRejectorSampleConsensus &other)
    : source_{other.source_}, target_{other.target_}, params{other.params}, best_{other.best_}, ctx{nullptr}, device{other.device} {}

template <typename PointT>
CorrespondenceRejectorSampleConsensus<PointT> &CorrespondenceRejectorSampleConsensus<PointT>::operator=(
    const CorrespondenceRejectorSampleConsensus &other) {
    if (this != &other) {
        source_ = other.source_;
        target_ = other.target_;
        params = other.params;
        best_ = other.best_;
        device = other.device;
    }
    return *this;
}

template <typename PointT>
CorrespondenceRejectorSampleConsensus<PointT>::~CorrespondenceRejectorSampleConsensus() {
    detail::corrRelease(this->ctx);
}

template <typename PointT>
void CorrespondenceRejectorSampleConsensus<PointT>::getRemainingCorrespondences(const std::vector<pcl::Correspondence> &original,
                                                                                std::vector<pcl::Correspondence> &remaining) {
    static_assert(sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) % 4 == 0,
                  "CorrespondenceRejectorSampleConsensus: a point type whose first three floats are x, y, z");
    double T[16];
    std::vector<pcl::Correspondence> kept;
    const bool found =
        detail::corrRansac(this->ctx, this->device, this->source_ ? this->source_->points.data() : nullptr,
                           this->source_ ? this->source_->points.size() : 0, this->target_ ? this->target_->points.data() : nullptr,
                           this->target_ ? this->target_->points.size() : 0, sizeof(PointT), this->params, original, kept, T);
    if (!found) {  // as PCL: the input and the identity
        kept = original;
        this->best_ = Eigen::Matrix4d::Identity();
    } else {
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) this->best_(r, c) = T[4 * r + c];
    }
    remaining.swap(kept);  // (`remaining` may be `original`)
}

}  // namespace wave

// PCL_INSTANTIATE_CorrespondenceRejectorSampleConsensus(MyPoint) in one source file of a program precompiles the class
#define PCL_INSTANTIATE_CorrespondenceRejectorSampleConsensus(T) template class wave::CorrespondenceRejectorSampleConsensus<T>;

#endif  // WAVE_CORRESPONDENCE_REJECTION_IMPL_HPP
