// pcl_filter_min.hpp -- the part of pcl::Filter<PointT> (PCL 1.8 filters/filter.h) that libwave's
// GroundSegmentation<PointT> is written against, for builds without PCL: setInputCloud / getInputCloud,
// filter() -- in place too, filter(*input) -- and pcl::copyPointCloud by indices (width = size, height = 1,
// is_dense from the input, as PCL sets them).  With PCL installed the real header is used.
#pragma once

#include "wave/compat/pcl_min.hpp"

#if defined(WAVE_MATCHING_USE_SYSTEM_PCL) || __has_include(<pcl/point_cloud.h>)
#include <pcl/common/io.h>
#include <pcl/filters/filter.h>
#else

#include <vector>

namespace pcl {

template <typename PointT>
void copyPointCloud(const PointCloud<PointT> &in, const std::vector<int> &indices, PointCloud<PointT> &out) {
    std::vector<PointT> pts(indices.size());
    for (size_t i = 0; i < indices.size(); ++i) pts[i] = in.points[static_cast<size_t>(indices[i])];
    const bool dense = in.is_dense;
    out.points.swap(pts);
    out.width = static_cast<uint32_t>(out.points.size());
    out.height = 1;
    out.is_dense = dense;
}

template <typename PointT>
class Filter {
 public:
    typedef pcl::PointCloud<PointT> PointCloud;
    typedef typename PointCloud::Ptr PointCloudPtr;
    typedef typename PointCloud::ConstPtr PointCloudConstPtr;

    virtual ~Filter() = default;
    virtual void setInputCloud(const PointCloudConstPtr &cloud) { input_ = cloud; }
    const PointCloudConstPtr getInputCloud() const { return input_; }

    // PCL: the output of a filter applied in place is formed aside and copied over the input afterwards
    void filter(PointCloud &output) {
        if (!input_) return;
        if (input_.get() == &output) {
            PointCloud tmp;
            applyFilter(tmp);
            output = tmp;
        } else {
            applyFilter(output);
        }
    }

 protected:
    PointCloudConstPtr input_;
    virtual void applyFilter(PointCloud &output) = 0;
};

}  // namespace pcl
#endif
